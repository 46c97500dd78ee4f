"""The host arithmetic of FGMRES (csrc/krylov_host.cpp: fg_restart_verdict, fg_column_step, fg_back_substitute) run alone, from
the stand-alone program tests/krylov_host_main.cpp built with the address and undefined-behaviour sanitizers.  No GPU needed: the
unit is plain C++ without the HIP runtime and without the solver object.

The input comes from the restatement tests/krylov_reference.py on the oracle's operators: fgmres (trace=...) records every true
residual norm and every Hessenberg column the host was handed, with what the restatement made of them.  The program gets the
same numbers and must take the same decisions (iteration count, end of cycle, breakdown, status, cycles per application,
stalled cycles, stagnation).  Its numbers are checked against what the arithmetic itself promises, not against another solver,
with u = 2^-53 and every product and sum on the checking side in np.longdouble:
  every rotation         |cs^2 + sn^2 - 1| <= 4 u
  back substitution      |H y - g| <= gamma_k |H| |y| componentwise, gamma_k = k u / (1 - k u), k columns, H the rotated upper
                         triangle (the backward error bound of substitution on a triangular system)
test_the_restatement_meets_the_bounds shows that the restatement's own numbers satisfy both on the same inputs.

What the runs cover is asserted in test_the_runs_cover_every_decision: a cycle that ends on the estimate, one that ends on the
column budget, a lucky breakdown (h[j+1] == 0), a weak-norm mark (negative sub-diagonal entry), a zero and a NaN column
(breakdown), three stalled cycles in a row (stagnation), the fallback to one cycle per application, the iteration budget."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import krylov_cases as kc
import krylov_reference as kr
from test_krylov_reference import oracle_operators

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
U = LD(2.0) ** -53


def _zero_precond(c):
    A, _ = oracle_operators(c, kc.NONE)
    return A, (lambda r: np.zeros_like(r))


def _nan_from_third_application(c):
    A, M = oracle_operators(c, kc.JACOBI)
    calls = []

    def sick(r):
        calls.append(1)
        return M(r) if len(calls) < 3 else np.full_like(r, np.nan)
    return A, sick


# name -> (case, operators, options of kr.fgmres)
RUNS = {
    # three restart cycles of 30 columns, then cycles that end on the estimate at the attainable accuracy: inner_scale goes down
    # to 1e-3, three cycles in a row gain less than 30 % and the guard stops the solve
    "n513-none-stagnates": ("n513", lambda c: oracle_operators(c, kc.NONE), dict(restart=30, max_iters=500, rtol=1e-18)),
    # two chained cycles per application until a restart cycle brings no progress; stopped by the iteration budget
    "n513-jacobi-steps2": ("n513", lambda c: oracle_operators(c, kc.JACOBI), dict(restart=8, max_iters=60, rtol=1e-18, precond_steps=2)),
    # a solve to 1e-10 that ends on the estimate inside its second cycle
    "n513-none-converges": ("n513", lambda c: oracle_operators(c, kc.NONE), dict(restart=30, max_iters=500, rtol=1e-10)),
    # the Krylov space closes at step 3: with one reduction per step the sub-diagonal entry is -0 there (lucky breakdown), and
    # later, at rounding level, negative (the weak-norm mark)
    "lucky513-one-reduce": ("lucky513", lambda c: oracle_operators(c, kc.NONE), dict(restart=30, max_iters=10, rtol=1e-18, pythagoras=True)),
    "n1-lucky": ("n1", lambda c: oracle_operators(c, kc.NONE), dict(restart=20, max_iters=1, rtol=1e-10)),
    "n513-zero-column": ("n513", _zero_precond, dict(restart=8, max_iters=20, rtol=1e-10)),
    "n513-nan-column": ("n513", _nan_from_third_application, dict(restart=8, max_iters=20, rtol=1e-10)),
}


@functools.lru_cache(maxsize=None)
def restated(name):
    case, operators, options = RUNS[name]
    c = kc.case(case)
    A, M = operators(c)
    trace = []
    with np.errstate(invalid="ignore"):
        res = kr.fgmres(A, M, c.b, trace=trace, **options)
    bnorm = math.sqrt(kr.Arith().dot(c.b, c.b))          # fg_begin of the restatement
    target = max(options["rtol"] * bnorm, 0.0)
    return res, trace, bnorm, target


# ---------------------------------------------------------------- the bounds
def check_rotations(cs, sn):
    cs, sn = np.asarray(cs, LD), np.asarray(sn, LD)
    dev = np.abs(cs * cs + sn * sn - LD(1.0))
    assert (dev <= 4 * U).all(), (float(dev.max()), float(4 * U))


def check_back_substitution(k, y, g, hcols):
    if k == 0:
        return
    H = np.zeros((k, k), LD)
    for c in range(k):
        H[:c + 1, c] = np.asarray(hcols[c], LD)
    y, g = np.asarray(y, LD), np.asarray(g[:k], LD)
    gamma = k * U / (LD(1.0) - k * U)
    lhs, rhs = np.abs(H @ y - g), gamma * (np.abs(H) @ np.abs(y))
    assert (lhs <= rhs).all(), (float((lhs - rhs).max()), k)


@pytest.mark.parametrize("name", sorted(RUNS))
def test_the_restatement_meets_the_bounds(name):
    _, trace, _, _ = restated(name)
    ends = [e for e in trace if e[0] == "end"]
    assert ends
    for _, k, y, cs, sn, g, hcols in ends:
        check_rotations(cs, sn)
        check_back_substitution(k, y, g, hcols)


def test_the_runs_cover_every_decision():
    def steps(name):
        return [e for e in restated(name)[1] if e[0] == "step"]

    def cycles(name):
        return [e for e in restated(name)[1] if e[0] == "cycle"]

    res = restated("n513-none-stagnates")[0]
    assert res.status == kr.NOT_CONVERGED and res.stagnated and res.inner_scale == 1e-3
    assert [e[2] for e in cycles("n513-none-stagnates")][-3:] == [0, 1, 2]                       # stalled cycles before the last restart
    est = [d for d in res.log if d.kind == "estimate"]
    assert any(d.taken for d in est)                                                             # a cycle that ends on the estimate
    ends = [e[1] for e in restated("n513-none-stagnates")[1] if e[0] == "end"]
    assert ends[:3] == [30, 30, 30] and not any(d.taken for d in est[:90])                       # three that end on the column budget
    res = restated("n513-jacobi-steps2")[0]
    assert res.status == kr.NOT_CONVERGED and not res.stagnated and res.iters == 60              # the iteration budget
    assert [e[1] for e in cycles("n513-jacobi-steps2")][:1] == [2] and cycles("n513-jacobi-steps2")[-1][1] == 1      # the fallback
    assert restated("n513-none-converges")[0].status == kr.OK and restated("n513-none-converges")[0].iters > 30
    h_last = [float(e[1][-1]) for e in steps("lucky513-one-reduce")]
    assert any(h == 0.0 for h in h_last) and any(h < 0.0 for h in h_last)                        # lucky breakdown, weak-norm mark
    assert [float(e[1][-1]) for e in steps("n1-lucky")] == [0.0] and restated("n1-lucky")[0].status == kr.OK
    zero = steps("n513-zero-column")
    assert len(zero) == 1 and zero[0][3] is None and not zero[0][1].any()                        # breakdown on a zero column
    nan = steps("n513-nan-column")
    assert len(nan) == 3 and nan[-1][3] is None and np.isnan(nan[-1][1]).all()                   # and on a NaN column, two columns in


# ---------------------------------------------------------------- the unit alone, under the sanitizers
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
# the sanitizer runtimes are linked into the program itself, so that it starts the same in whatever environment it inherits
STATIC_RUNTIME = ["-static-libasan", "-static-libubsan"]


@pytest.fixture(scope="module")
def sanitized_program(tmp_path_factory):
    """csrc/krylov_host.cpp + tests/krylov_host_main.cpp as one program: the unit links without the HIP runtime and without any
    other unit of the library."""
    d = tmp_path_factory.mktemp("krylov_host_asan")
    probe = d / "probe.cpp"
    probe.write_text("int main () { return 0; }\n")
    if subprocess.run(["g++", "-fsanitize=address", *STATIC_RUNTIME, str(probe), "-o", str(d / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler cannot link -fsanitize=address")
    exe = str(d / "krylov_host_main")
    cxx = ["g++", "-std=c++17", "-Wall", "-ffp-contract=off", *SANITIZE]
    units = [os.path.join(ROOT, "tests", "krylov_host_main.cpp"), os.path.join(ROOT, "nk_ocn_tracer_jacobian_precond_amd", "csrc", "krylov_host.cpp")]
    objs = [str(d / (os.path.basename(u) + ".o")) for u in units]
    jobs = [subprocess.Popen([*cxx, "-c", u, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for u, o in zip(units, objs)]
    for j in jobs:                                   # any warning fails the build
        out = j.communicate()[0]
        assert j.returncode == 0 and not out.strip(), out
    r = subprocess.run([*cxx, *STATIC_RUNTIME, *objs, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    return exe


def _hex(v):
    return "nan" if v != v else float(v).hex()


def _floats(words):
    return [float.fromhex(w) for w in words]


@pytest.mark.parametrize("name", sorted(RUNS))
def test_host_unit_under_sanitizers(name, sanitized_program, tmp_path):
    res, trace, bnorm, target = restated(name)
    options = RUNS[name][2]
    m = options["restart"]
    lines = [f"{m} {options['max_iters']} {options.get('precond_steps', 1)} {_hex(bnorm)} {_hex(target)}"]
    for e in trace:
        if e[0] == "restart":
            lines.append("R " + _hex(e[1]))
        elif e[0] == "step":
            lines.append("S " + " ".join(_hex(h) for h in e[1]))
        elif e[0] == "end":
            lines.append("E")
    path = tmp_path / "solve.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([sanitized_program, str(path)], capture_output=True, text=True, timeout=60)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "runtime error" not in out and "AddressSanitizer" not in out, out
    got = [ln.split() for ln in r.stdout.splitlines()]
    pos = 0
    for i, e in enumerate(trace):
        key, *w = got[pos]
        if e[0] == "restart":
            assert key == "restart"
            todo, finished, status, steps_now, stalled = (int(v) for v in w[:5])
            relres, inner_scale = _floats(w[5:])
            goes_on = i + 1 < len(trace) and trace[i + 1][0] == "cycle"
            assert finished == (0 if goes_on else 1) and bool(todo & 1) == (not goes_on)
            assert relres == e[1] / bnorm
            if goes_on:
                assert (steps_now, stalled) == trace[i + 1][1:3], (i, got[pos], trace[i + 1])
                assert bool(todo & 2) == (i > 0 and steps_now == 1 and [c for c in trace[:i] if c[0] == "cycle"][-1][1] > 1)
                assert not todo & 4
            else:
                # the last restart: the verdict of the solve (NKP_OK, NKP_NOT_CONVERGED and NKP_BREAKDOWN are the restatement's codes)
                assert i == len(trace) - 1 and status == res.status and bool(todo & 4) == res.stagnated
            assert 1e-3 <= inner_scale <= 1.0
            pos += 1
        elif e[0] == "cycle":
            continue
        elif e[0] == "step":
            assert key == "step"
            its, ends, breakdown = (int(v) for v in w[:3])
            assert (its, bool(ends), bool(breakdown)) == (e[2], bool(e[4]), e[3] is None), (i, got[pos], e[2:])
            pos += 1
        else:
            assert key == "end" and int(w[0]) == e[1]
            k = e[1]
            rows = {g[0]: _floats(g[1:]) for g in got[pos + 1:pos + 6]}
            assert sorted(rows) == ["H", "cs", "g", "sn", "y"] and [len(rows[q]) for q in ("y", "cs", "sn", "g", "H")] == [k, k, k, k + 1, k * (k + 1) // 2]
            hcols, at = [], 0
            for c in range(k):
                hcols.append(rows["H"][at:at + c + 1])
                at += c + 1
            check_rotations(rows["cs"], rows["sn"])
            check_back_substitution(k, rows["y"], rows["g"], hcols)
            pos += 6
    assert pos == len(got)
    if trace[-1][0] == "end":
        # the solve ended in a breakdown inside a cycle: fg_column_step said so, and the true residual of what was there decided
        assert [e for e in trace if e[0] == "step"][-1][3] is None
    else:
        assert res.iters == [e for e in trace if e[0] == "step"][-1][2] if any(e[0] == "step" for e in trace) else res.iters == 0


# ---------------------------------------------------------------- the verdict on the right-hand side
FLOOR = 2.0 ** -480          # NKP_TARGET_FLOOR (krylov_host.h); 2^-960 for its square is 62 binary orders above the smallest normal
ORDINARY, ZERO, NONFINITE, OUT_OF_RANGE = kr.RHS_ORDINARY, kr.RHS_ZERO, kr.RHS_NONFINITE, kr.RHS_OUT_OF_RANGE
SUBNORMAL = 2.0 ** -1070
# (||b||^2, target, non-finite entries, entries != 0) -> (the entries are counted, verdict).  The expectation is the contract of
# include/nkp.h written out by hand, not a call of the restatement.
VERDICTS = [
    ((4.0, 2e-10, 0, 7), (0, ORDINARY)),
    ((4.0, 2e-10, 3, 0), (0, ORDINARY)),                       # inside the range the counts are not looked at
    ((0.0, 0.0, 0, 0), (1, ZERO)),                             # b = 0
    ((0.0, 0.0, 0, 5), (1, OUT_OF_RANGE)),                     # every square underflowed: b 2^-600
    ((0.0, 0.0, 2, 5), (1, NONFINITE)),
    ((SUBNORMAL, 1e-10 * math.sqrt(SUBNORMAL), 0, 513), (1, OUT_OF_RANGE)),
    ((SUBNORMAL, 1e-10 * math.sqrt(SUBNORMAL), 0, 0), (1, ZERO)),       # (not reachable: a count that contradicts the norm)
    ((math.inf, math.inf, 0, 513), (1, OUT_OF_RANGE)),         # b 2^520: finite entries, ||b||^2 overflows
    ((math.inf, math.inf, 1, 513), (1, NONFINITE)),            # +Inf in b
    ((math.inf, math.inf, 513, 513), (1, NONFINITE)),
    ((math.nan, 0.0, 1, 513), (1, NONFINITE)),                 # NaN in b; fmax (rtol NaN, atol = 0) = 0
    ((math.nan, 1e-8, 2, 513), (1, NONFINITE)),                # ... and with atol > 0: the norm alone sends it to the counts
    ((math.nan, math.nan, 1, 1), (1, NONFINITE)),
    ((1.0, math.nextafter(FLOOR, 0.0), 0, 9), (1, OUT_OF_RANGE)),      # the target just below 2^-480
    ((1.0, FLOOR, 0, 9), (0, ORDINARY)),                       # at it
    ((1.0, math.nextafter(FLOOR, 1.0), 0, 9), (0, ORDINARY)),  # just above
    ((2.0 ** -1000, 1e-8, 0, 9), (0, ORDINARY)),               # atol > 0 keeps a tiny b on the normal path
    ((SUBNORMAL, 1e-8, 0, 9), (0, ORDINARY)),
    ((0.0, 1e-8, 0, 9), (0, ZERO)),                            # ... and where its squares are all gone, ||b|| < atol: x = 0 meets it
    ((0.0, 1e-8, 0, 0), (0, ZERO)),
]


def test_rhs_verdict_of_the_restatement():
    for (bnorm2, target, nonfinite, nonzero), (counts, verdict) in VERDICTS:
        assert kr.rhs_needs_counts(bnorm2, target) == bool(counts), (bnorm2, target)
        assert kr.rhs_verdict(bnorm2, target, nonfinite, nonzero) == verdict, (bnorm2, target, nonfinite, nonzero)


def test_rhs_verdict_under_sanitizers(sanitized_program, tmp_path):
    lines = ["1 0 1 0x1p+0 0x0p+0"] + ["V " + " ".join(_hex(float(v)) for v in args) for args, _ in VERDICTS]
    path = tmp_path / "verdicts.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([sanitized_program, str(path)], capture_output=True, text=True, timeout=60)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "runtime error" not in out and "AddressSanitizer" not in out, out
    got = [tuple(int(v) for v in ln.split()[1:]) for ln in r.stdout.splitlines()]
    assert all(ln.startswith("verdict ") for ln in r.stdout.splitlines())
    assert got == [want for _, want in VERDICTS], list(zip(VERDICTS, got))


def test_a_non_finite_restart_is_a_breakdown_without_a_relres(sanitized_program, tmp_path):
    """fg_restart_verdict with beta = Inf (a start vector with an Inf) and NaN: NKP_BREAKDOWN, relres NaN"""
    for beta in ("inf", "nan"):
        path = tmp_path / f"restart_{beta}.txt"
        path.write_text(f"4 10 1 0x1p+0 0x1p-30\nR {beta}\n")
        r = subprocess.run([sanitized_program, str(path)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and not r.stderr.strip(), r.stdout + r.stderr
        w = r.stdout.split()
        assert w[0] == "restart" and int(w[1]) & 1 and int(w[2]) == 1 and int(w[3]) == kr.BREAKDOWN and "nan" in w[6].lower(), r.stdout
