"""Forward mode of NkpTorchSolver.solve: torch.autograd.forward_ad dual tensors run nkp_solve_tangent_device.

The tangent has the bits of the call it is made of, a dual on B alone makes no product with the values, the reverse mode is
unchanged by save_for_forward, and the two modes agree on the golden fixtures within a derived bound.  torch runs in a process of
its own (it brings its own HIP runtime along): tests/torch_forward_mode_worker.py."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fwd") / "torch.json")
    env = dict(os.environ, NKP_ML_DEVICE_MIN="0", NKP_ML_COARSEST_ROWS="300")
    r = subprocess.run([sys.executable, os.path.join(HERE, "torch_forward_mode_worker.py"), "--out", out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.load(open(out))


def test_tangent_has_the_bits_of_the_tangent_solve(result):
    for name in ("dual_B", "dual_val", "dual_both"):
        c = result[name]
        assert c["has_tangent"] and c["equal"] and c["tangent_calls"] == 1, (name, c)
    assert result["no_dual_no_tangent"], result


def test_a_dual_on_B_alone_makes_no_product_with_the_values(result):
    assert result["dual_B"]["product_calls"] == 0, result["dual_B"]
    assert result["dual_val"]["product_calls"] == 1 and result["dual_both"]["product_calls"] == 1, result


def test_backward_is_bit_identical_with_and_without_save_for_forward(result):
    assert result["backward_unchanged"], result


def test_a_tangent_solve_that_does_not_converge_raises(result):
    assert result["not_converged_raises"], result


def test_a_right_hand_side_with_a_nan_raises(result):
    """NkpTorchSolver.solve of a B with one NaN row: NkpError (NKP_BREAKDOWN, "holds a non-finite entry"), no tensor"""
    assert result["nan_row_raises"], result


def test_forward_and_reverse_mode_agree_on_the_golden_fixtures(result):
    """<W, jvp (dB, dval)> against <B.grad, dB> + <val.grad, dval>, K = 2, the solver options of the existing value-gradient test.

    Both modes use the SAME computed X: the reverse mode gives <Lam, dB> - <Lam, dA X> = <Lam, R> with R = dB - dA X, the forward
    mode <W, dX> with dX the computed A^-1 R, and exactly <W, A^-1 R> = <A^-T W, R>.  So the difference is
        <W, dX - A^-1 R> + <A^-T W - Lam, R>
    As in the directional bound of tests/test_gpu_value_gradient.py, the library's solves (A and A^T, rtol = 1e-12) agree with a
    direct solve to 1e-7 in the 2-norm, relative to the solution (the bound test_solve_matches_superlu_fixture asserts), so by
    Cauchy-Schwarz per right-hand side
        |difference| <= 1e-7 sum_c (||W_c|| ||dX_c|| + ||Lam_c|| ||R_c||)
    The roundings of the product, the gradient and the inner products are nine orders below that and are not added."""
    assert len(result["consistency"]) == 4
    for c in result["consistency"]:
        bound = 1e-7 * sum(c["norm_W"][k] * c["norm_dX"][k] + c["norm_Lam"][k] * c["norm_R"][k] for k in range(2))
        diff = abs(c["forwards"] - c["backwards"])
        print(f"{c['name']}: forwards {c['forwards']:.17g}, backwards {c['backwards']:.17g}, difference {diff:.3e}, bound {bound:.3e}")
        assert diff <= bound, c
