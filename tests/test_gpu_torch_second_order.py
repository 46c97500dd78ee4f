"""Second derivatives through NkpTorchSolver.solve: the backward pass is made of five operations that differentiate each other
(torch_op.py), the one the library lacked being nkp_values_product_trans.

A Hessian-vector product has the bits of the chain of library calls it is documented to be and makes the documented calls; a
plain backward is unchanged and leaves no graph; the result agrees with torch's own double differentiation of a dense solve within
a derived bound; an inner solve that does not converge raises.  torch runs in a process of its own (it brings its own HIP runtime
along): tests/torch_second_order_worker.py."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 1e-7          # what test_solve_matches_superlu_fixture asserts of a solve, relative to the solution in the 2-norm


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("second") / "torch.json")
    env = dict(os.environ, NKP_ML_DEVICE_MIN="0", NKP_ML_COARSEST_ROWS="300")
    r = subprocess.run([sys.executable, os.path.join(HERE, "torch_second_order_worker.py"), "--out", out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.load(open(out))


def test_hessian_vector_product_has_the_bits_of_the_chain_of_library_calls(result):
    """(hB, hval, hW) = grad (<P, gB> + <q, gval>, (B, val, W)), (gB, gval) = grad (<W, X>, (B, val), create_graph = True), against
    Lambda = A^-T W; U = -Q X; Xbar = -Q^T Lambda; M = A^-1 (P + U); Lambda2 = A^-T Xbar; hW = M; hB = Lambda2;
    hval = -vg (Lambda, M) + -vg (Lambda2, X), made directly from the library calls and the same torch adds"""
    c = result["composition"]
    assert c["nonzero"] and c["hB"] and c["hval"] and c["hW"], c


def test_one_hessian_vector_product_makes_four_solves_and_one_transposed_product(result):
    assert result["calls"] == dict(solves=2, transposed_solves=2, value_gradients=3, products=1, products_trans=1), result["calls"]


def test_first_order_gradients_keep_their_bits_and_leave_no_graph(result):
    f = result["first_order"]
    assert f["B"] and f["val"] and f["no_graph"], f
    assert f["calls"] == dict(solves=1, transposed_solves=1, value_gradients=1, products=0), f["calls"]


def test_double_backward_whose_inner_solve_does_not_converge_raises(result):
    assert result["not_converged_raises"], result


def test_second_derivatives_agree_with_torch_on_the_dense_matrix(result):
    """Every golden fixture, K = 2, rtol = 1e-12: hB, hval, hW against torch.autograd.grad twice through torch.linalg.solve on the
    dense A (val), float64 on the CPU, in the 2-norm (Frobenius over the two vectors).

    Exactly, with Q the matrix of q on A's pattern, X = A^-1 B, Lam = A^-T W:
        M = A^-1 (P - Q X) = hW,      Lam2 = A^-T (- Q^T Lam) = hB,      hval = - vg (Lam, M) - vg (Lam2, X),   vg (a, b)[e] = sum_c a_c[row e] b_c[col e]
    The code computes the same chain, and what separates it from these is the error of its four solves; the products and gradients on
    the pattern round at 1e-16 per term, nine orders below, and are not added -- nor is the error of the dense side, cond (A) 1e-16.
    As in test_forward_and_reverse_mode_agree_on_the_golden_fixtures, a solve of the library (A or A^T) agrees with the exact
    solution OF THE RIGHT-HAND SIDE IT WAS GIVEN to eps = 1e-7 relative in the 2-norm (the bound test_solve_matches_superlu_fixture
    asserts).  To first order in eps:
        ||dX|| <= eps ||X||,   ||dLam|| <= eps ||Lam||
        the right-hand side of M is off by Q dX:          ||dM||    <= eps (||M|| + ||A^-1 Q||_2 ||X||)
        the right-hand side of Lam2 is off by Q^T dLam:   ||dLam2|| <= eps (||Lam2|| + ||Q A^-1||_2 ||Lam||)      (||A^-T Q^T|| = ||Q A^-1||)
    (the products A^-1 Q and Q A^-1 are not split into ||A^-1|| ||Q||: q is of the size of the values, so they are of order one while
    ||A^-1||_2 ||A||_2 is 1e6 .. 1e7 here, and the split bound would exceed the result itself)
        ||vg (a, b)||_2 <= ||sum_c a_c b_c^T||_F <= ||a||_F ||b||_F on a pattern without repeated entries (asserted by the worker), so
        ||dhval|| <= ||dLam|| ||M|| + ||Lam|| ||dM|| + ||dLam2|| ||X|| + ||Lam2|| ||dX||
    and the terms of second order in eps are covered by the factor 1.01.  Every norm on the right is taken on the dense side (numpy);
    nothing measured on the code under test enters.  A sign or transpose error shows as a difference of the order of the result."""
    assert len(result["dense"]) == 4
    for c in result["dense"]:
        N = c["norm"]
        dX, dLam = EPS * N["X"], EPS * N["Lam"]
        dM = EPS * (N["M"] + N["AinvQ"] * N["X"])
        dLam2 = EPS * (N["Lam2"] + N["QAinv"] * N["Lam"])
        bound = dict(hW=1.01 * dM, hB=1.01 * dLam2, hval=1.01 * (dLam * N["M"] + N["Lam"] * dM + dLam2 * N["X"] + N["Lam2"] * dX))
        for k in ("hB", "hval", "hW"):
            print(f"{c['name']} {k}: |difference| / |dense| = {c['diff'][k] / c['ref'][k]:.3e}, bound / |dense| = {bound[k] / c['ref'][k]:.3e}"
                  f"  (||A^-1|| {N['Ainv']:.3e}, ||A|| {N['A']:.3e}, ||A^-1 Q|| {N['AinvQ']:.3e}, ||Q A^-1|| {N['QAinv']:.3e})")
        for k in ("hB", "hval", "hW"):                              # the closed forms above are what torch differentiates to: the dense side
            assert c["closed_form"][k] <= 1e-8, (c["name"], k, c["closed_form"])      # alone, cond (A) 2^-52 = 3e-9 at most here
        for k in ("hB", "hval", "hW"):
            assert c["diff"][k] <= bound[k], (c["name"], k, c["diff"][k], bound[k])
