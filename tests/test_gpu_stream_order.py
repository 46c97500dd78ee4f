"""nkp_set_stream: every device entry point on a caller's stream behind pending work.

torch's side streams and the solver's own stream are non-blocking, so nothing orders the null stream -- where every synchronous
hipMemcpy / hipMemset runs -- with the caller's work; the rest of the suite calls the library on the null stream or on the
solver's own idle one, where a kernel on the wrong stream or a copy made too early still gives the right answer.

The detector is a late producer (tests/stream_order_worker.py): an operand is filled with NaN, and on the stream S the solver was
given a sleep kernel, the copy of the true values and an event are enqueued; the library is called at once.  A reader anywhere but
in order on S reads NaN: a wrong result, NKP_BREAKDOWN or a refused refactor (all operands are doubles, no index array is passed by
device pointer).  The result of each call is read back on a stream that is not ordered with S, without a synchronisation of
torch's: it must be complete when the call returns.  Expected are the bits of the same program of calls on fresh solvers that
never saw set_stream, with torch.cuda.synchronize () around every call -- the library's determinism is asserted throughout the
suite -- and one product is anchored outside the library, on the numpy oracle of the SpMV tests.

A call whose producer had already finished when the library was entered has tested nothing: that fails
test_the_detector_sees_and_every_call_was_entered_early, as does a control reader on another stream that does not see the NaN.

The solvers: the matrix and hierarchy of tests/test_gpu_step_glue.py (lane-per-column and wave-per-column levels, a dense last
level); M = multilevel with FGMRES on an f64 basis, J = column Jacobi with an f32 basis, whose batched entry solves one at a time.
A one-rank row-distributed solver on the file transport runs the single solves.  Row-distributed solvers of more than one rank
are out of scope: their collectives stay on the solver's own stream (tests/dist_worker.py)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

# late calls per numbered case of the worker's program
CALLS = {1: 1, 2: 4, 3: 4, 4: 2, 5: 13, 6: 2, 7: 3, 8: 7, 9: 3, 10: 1, 11: 4, 12: 1, 13: 5, 14: 2}


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("stream_order") / "stream_order.json")
    r = subprocess.run([sys.executable, os.path.join(HERE, "stream_order_worker.py"), "--out", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.load(open(out))


def describe(c):
    if c["error"]:
        return f"{c['name']}: {c['entry']} on {c['solver']} with a late {c['operand']} raised\n{c['error']}"
    return (f"{c['name']}: {c['entry']} on {c['solver']} with a late {c['operand']}: {c['differ']} of {c['total']} doubles differ from the expected bits; "
            f"answered {c['ret']}, expected {c['ret_expected']}")


def check(result, case):
    cases = [c for c in result["cases"] if c["case"] == case]
    assert len(cases) == CALLS[case], (case, [c["name"] for c in cases])
    bad = [describe(c) for c in cases if c["error"] or not (c["equal"] and c["ret_equal"])]
    assert not bad, "\n".join(bad)
    assert not [c["name"] for c in cases if c["total"] == 0 and c["ret"] is None and not c["name"].startswith("wrapper set_values")]
    return {c["name"]: c for c in cases}


def test_the_detector_sees_and_every_call_was_entered_early(result):
    """The control: a clone made on a second non-blocking stream while S sleeps in front of the copy must contain NaN, or the delay
    is too short to detect anything.  The per-call condition: the producer's event had not completed immediately before each of
    the library calls -- for every call, none left out."""
    print(f"torch.cuda._sleep ({result['sleep_cycles']}) measured {result['sleep_ms']:.2f} ms on the solver's stream "
          f"(10 000 000 cycles: {result['probe_ms']:.2f} ms); {len(result['cases'])} late calls")
    assert not result["expected_errors"], result["expected_errors"]
    ctl = result["control"]
    assert ctl["late_values_arrived"], ctl
    assert ctl["unfinished_at_read"] and ctl["clone_saw_nan"], f"delay too short to detect anything: {ctl}, sleep {result['sleep_ms']:.2f} ms"
    assert len(result["cases"]) == sum(CALLS.values()) == result["expected_calls"]
    finished = [c["name"] for c in result["cases"] if not c.get("unfinished_at_entry")]
    assert not finished, f"the producer had finished when the library was entered (these calls tested nothing): {finished}"
    h = result["hierarchy"]
    print("levels", h["levels"], "(wave_columns, lane_diag) per smoothed level", h["kinds"], "dense last", h["dense_last"], "n", result["n"])
    assert h["levels"] >= 4 and h["dense_last"]
    assert any(w == 0 for w, _ in h["kinds"]) and any(w == 1 for w, _ in h["kinds"])


def test_spmv_device_reads_a_late_x(result):
    check(result, 1)
    assert result["spmv_late_x_has_the_oracle_bits"]


def test_solve_device_reads_a_late_b_and_a_late_guess(result):
    c = check(result, 2)
    assert c["solve late b on M"]["ret"][0][0] == 0 and c["solve late b on M"]["ret"][0][1] > 5, c["solve late b on M"]["ret"]


def test_solve_batch_device_creates_and_reuses_its_members_behind_a_late_B(result):
    c = check(result, 3)
    ret = c["solve_batch late B on M, first call (creates the members)"]["ret"]
    assert len(ret) == 3 and all(r[0] == 0 and r[1] > 5 for r in ret), ret


def test_solve_batch_device_ex_reads_a_late_B_and_late_guesses(result):
    c = check(result, 4)
    ret = c["solve_batch_ex late X"]["ret"]
    assert all(r[0] == 0 for r in ret) and ret[0][1] < ret[2][1], ret          # rtol 1e-6 against 1e-8: the columns' own controls ran


def test_refactor_device_reads_late_values_and_every_handle_follows(result):
    """flags 0 and a rebuild, without a transposed handle and with the handle and the batch members of both alive: the solve, the
    batched solve on remade members and the batched solve on the transposed handle after it"""
    check(result, 5)
    assert result["refactor_rebuilt"] == [0, 1, 0, 1], result["refactor_rebuilt"]
    assert result["same_transposed_handle"]


def test_transposed_handle_built_before_and_after_set_stream_reads_a_late_G(result):
    check(result, 6)


def test_value_gradient_device_reads_late_vectors_and_a_late_g(result):
    check(result, 7)


def test_values_products_read_late_values_and_vectors(result):
    check(result, 8)
    assert result["trans_index"]["before"] == 0 and result["trans_index"]["after"] > 0, result["trans_index"]      # the first call built the index


def test_solve_tangent_device_reads_late_operands(result):
    check(result, 9)


def test_a_clone_is_given_the_stream(result):
    assert result["clone_set_stream"] is True, result["clone_set_stream"]
    check(result, 10)


def test_members_and_transposed_handle_move_with_the_solver(result):
    """set_stream to a third stream with S idle -- a member left behind on S would run ahead of its operands -- then to the null
    stream, the producer on torch's default stream"""
    m = result["before_move"]
    assert m["batch_member_bytes"] > 0 and m["transposed_batch_member_bytes"] > 0, m
    check(result, 11)


def test_the_stream_stays_usable_after_a_breakdown(result):
    assert result["nan_b_status"] == 2, result["nan_b_status"]          # NKP_BREAKDOWN for a right-hand side that really is NaN
    check(result, 12)


def test_the_torch_wrapper_on_a_side_stream(result):
    """NkpTorchSolver constructed under torch.cuda.stream (S): set_values, solve, backward (the transposed handle is born inside
    it), a Hessian-vector product and a forward-mode tangent, each with a late operand, against the same program on the default
    stream with synchronisation"""
    assert result["transposed_before_backward"] is False and result["transposed_after_backward"] is True
    check(result, 13)


def test_a_one_rank_row_distributed_solver_on_a_side_stream(result):
    """force_dist = 1 on the file transport: the single solves of case 2 through the row-distributed drivers (their exchanges and
    reductions name the solver's stream to the transport)"""
    check(result, 14)
    assert result["one_rank_allreduce_calls"] > 0, result["one_rank_allreduce_calls"]
