"""Host-side aggregation of the multilevel preconditioner (nkp_ml_plan_host, csrc/ml_plan.cpp) against the
independent scipy restatement tests/ml_reference.py: identical coarse cells and coarse columns on every level, at the default
knobs and under every option of the aggregation (the cases of tests/ml_setup_cases.py, both sides under the same knobs); against
recorded hashes on hierarchies of several levels, with and without grid positions; and once more from a stand-alone
program built with the address and undefined-behaviour sanitizers.  No GPU needed: the plan is host code, compiled by
the host compiler."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import ml_reference as mlr
import ml_setup_cases as msc
from ml_structure_checks import same_partition as _same_partition
from nk_ocn_tracer_jacobian_precond_amd import solver, synth


@pytest.mark.parametrize("grid,refine,k33", [((24, 20, 10), 1.0, False), ((40, 46, 20), 1.0, False), ((40, 46, 20), 12.0, True),
                                            ((64, 60, 30), 12.0, False)])
def test_split_aggregation_matches_restatement(grid, refine, k33):
    p = synth.generate(imt=grid[0], jmt=grid[1], km=grid[2], adv="upwind3", hmix="isop", seed=2, u_scale=3.0 * refine,
                       ah=4.0e6 * refine ** 2, isop_k33=k33)
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    colid = np.cumsum(p.ind_k == 0) - 1
    levels = mlr.build(p.scipy_csr(), p.ind_i.astype(np.int64), p.ind_j.astype(np.int64), p.ind_k.astype(np.int64), colid)
    rows, cmaps, colofs = solver.ml_plan_host(p.rowptr, p.colind, p.nzval, blk, ci, cj)
    assert list(rows) == [lv.n for lv in levels]
    # the product numbers coarse rows differently: compare through the fine level
    to_ref = np.arange(p.flat_len)          # product row of level l -> restatement row of level l
    for l in range(len(levels) - 1):
        ref_of_fine = levels[l].cmap[to_ref]                      # restatement's coarse row of every product row
        assert _same_partition(cmaps[l], ref_of_fine), f"coarse cells differ on level {l}"
        nxt = np.empty(rows[l + 1], np.int64)
        nxt[cmaps[l]] = ref_of_fine
        to_ref = nxt
        assert _same_partition(colofs[l], levels[l].coarse_colid[to_ref]), f"coarse columns differ on level {l + 1}"


# ---------------------------------------------------------------- every option of the aggregation (tests/ml_setup_cases.py)
@pytest.fixture(scope="module")
def restated_plans():
    """ml_reference.build of a case under the case's knobs, built once"""
    cache = {}

    def get(case):
        if case not in cache:
            c = msc.CASES[case]
            p, blk, ci, cj, col_t = msc.problem(case)
            ri, rj, rk, colid, tracer = msc.row_arrays(blk, ci, cj, c.cnt, col_t)
            cache[case] = mlr.build(p.scipy_csr(), ri, rj, rk, colid, tracer=tracer if c.cnt > 1 else None, **msc.restatement_knobs(case))
        return cache[case]
    return get


def _cells(levels):
    """the coarse cells of every step as sets of level-0 rows: comparable between hierarchies of the same matrix"""
    out, to_fine = [], np.arange(levels[0].n)
    for lv in levels[:-1]:
        to_fine = lv.cmap[to_fine]
        out.append(to_fine.copy())
    return out


# nkp_ml_plan_host names no tracer per column, so the cell-major cases are left to the GPU tests; the tracer-major ones go
# beyond the single-tracer cases and check the restatement's rule for coupled tracers
@pytest.mark.parametrize("case", [n for n in msc.names() if not msc.CASES[n].cell_major])
def test_plan_options_match_restatement(case, restated_plans, monkeypatch):
    c = msc.CASES[case]
    p, blk, ci, cj, _ = msc.problem(case)
    levels = restated_plans(case)
    msc.setenv(case, monkeypatch)
    rows, cmaps, colofs = solver.ml_plan_host(p.rowptr, p.colind, p.nzval, blk, ci, cj, coupled_tracer_cnt=c.cnt, coarsest_rows=msc.coarsest_rows(case))
    print(case, "rows per level", list(rows), "counts", [lv.counts for lv in levels[:-1]])
    assert [lv.n for lv in levels] == c.rows
    assert list(rows) == c.rows
    if c.rows200:                                   # the same hierarchy cut off at 200 rows
        cut = next(l for l, n in enumerate(c.rows) if n <= 200) + 1
        assert c.rows[:cut] == c.rows200
    to_ref = np.arange(p.flat_len)
    for l in range(len(levels) - 1):
        ref_of_fine = levels[l].cmap[to_ref]
        assert _same_partition(cmaps[l], ref_of_fine), f"coarse cells differ on level {l}"
        nxt = np.empty(rows[l + 1], np.int64)
        nxt[cmaps[l]] = ref_of_fine
        to_ref = nxt
        assert _same_partition(colofs[l], levels[l].coarse_colid[to_ref]), f"coarse columns differ on level {l + 1}"


def test_plan_option_cases_reach_their_branches(restated_plans):
    """the conditions under which the cases above mean something, from the restatement's own counts"""
    count = lambda case, what: sum(lv.counts[what] for lv in restated_plans(case)[:-1])
    single = [n for n in msc.names(single_tracer=True) if msc.CASES[n].group != "stall"]
    assert any(count(n, "leaf_stubs") > 0 for n in single)
    assert count("tau0", "leaf_stubs") == 0
    assert any(count(n, "pockets_merged") > 0 for n in single)
    assert count("pocket0", "pockets_merged") == 0
    assert count("default", "leaf_stubs") > 0 and count("default", "pockets_merged") > 0     # so tau0 and pocket0 switch something off
    default = _cells(restated_plans("default"))
    for case in ("tau0", "tau0.2", "pocket0", "pocket9"):
        cells = _cells(restated_plans(case))
        assert len(cells) != len(default) or any(not _same_partition(a, b) for a, b in zip(cells, default)), case
    for case in msc.names("depth"):
        _, blk, _, _, _ = msc.problem(case)
        assert np.diff(blk).max() >= 64, case
    for case in msc.names("ties"):
        print(case, "absorbed stubs whose anchor the tie rule chose:", count(case, "anchor_ties"))
    assert any(count(case, "anchor_ties") > 0 for case in msc.names("ties"))
    assert [lv.n for lv in restated_plans("stall")] == [383] and [lv.n for lv in restated_plans("near_stall")] == [383, 381]


# ---------------------------------------------------------------- recorded plans (tests/golden/ml_plan_sha256.json)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_GRIDS = [((12, 10, 6), 1.0, False), ((24, 20, 10), 1.0, False), ((40, 46, 20), 12.0, True)]
PLAN_CASES = [(g, r, k, geo) for g, r, k in PLAN_GRIDS for geo in (True, False)]
PLAN_ROWS = {"12x10x6-geo": [383, 150], "12x10x6-graph": [383, 117],
             "24x20x10-geo": [2813, 889, 275, 100], "24x20x10-graph": [2813, 767, 233, 82],
             "40x46x20-geo": [21952, 6198, 1830, 529, 103], "40x46x20-graph": [21952, 5848, 1629, 510, 191]}


def _case_name(grid, geo):
    return "x".join(map(str, grid)) + ("-geo" if geo else "-graph")


def _plan_input(grid, refine, k33):
    p = synth.generate(imt=grid[0], jmt=grid[1], km=grid[2], adv="upwind3", hmix="isop", seed=2, u_scale=3.0 * refine,
                       ah=4.0e6 * refine ** 2, isop_k33=k33)
    blk = solver.column_blocks(p.col_start(), p.tracer_state_len, 1)
    ci, cj = solver.column_coords(p.ind_i, p.ind_j, p.col_start(), 1)
    return p, blk, ci, cj


def _sha(a, dtype):
    return hashlib.sha256(np.ascontiguousarray(a, dtype).tobytes()).hexdigest()


def plan_sha256(grid, refine, k33, geo):
    """rows per level and the sha256 of rows (int64), every cmap and every col_of (int32) of the plan at coarsest_rows = 200"""
    p, blk, ci, cj = _plan_input(grid, refine, k33)
    rows, cmaps, colofs = solver.ml_plan_host(p.rowptr, p.colind, p.nzval, blk, ci if geo else None, cj if geo else None, coarsest_rows=200)
    return {"rows": [int(r) for r in rows], "sha256": {"rows": _sha(rows, np.int64), "cmap": [_sha(c, np.int32) for c in cmaps],
                                                       "col_of": [_sha(c, np.int32) for c in colofs]}}


@pytest.fixture(scope="module")
def recorded_plans():
    with open(os.path.join(ROOT, "tests", "golden", "ml_plan_sha256.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("grid,refine,k33,geo", PLAN_CASES)
def test_plan_equals_recorded(grid, refine, k33, geo, recorded_plans):
    name = _case_name(grid, geo)
    got = plan_sha256(grid, refine, k33, geo)
    assert got["rows"] == PLAN_ROWS[name]
    assert got == recorded_plans[name]


# ---------------------------------------------------------------- the planner alone, under the sanitizers
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
# the sanitizer runtimes are linked into the program itself, so that it starts the same in whatever environment it inherits
STATIC_RUNTIME = ["-static-libasan", "-static-libubsan"]


@pytest.fixture(scope="module")
def sanitized_planner(tmp_path_factory):
    """tuning.cpp + ml_plan.cpp + dist_plan.cpp + tests/ml_plan_main.cpp as one program: the host units link without the HIP
    runtime and without solver.o.  All six inputs have fewer than 200000 rows, below which for_row_chunks stays on the calling
    thread: the run covers the planner's index arithmetic, not its row-parallel loops on more than one thread."""
    d = tmp_path_factory.mktemp("ml_plan_asan")
    probe = d / "probe.cpp"
    probe.write_text("int main () { return 0; }\n")
    if subprocess.run(["g++", "-fsanitize=address", *STATIC_RUNTIME, str(probe), "-o", str(d / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler cannot link -fsanitize=address")
    csrc = os.path.join(ROOT, "nk_ocn_tracer_jacobian_precond_amd", "csrc")
    exe = str(d / "ml_plan_main")
    cxx = ["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", *SANITIZE]
    units = [os.path.join(ROOT, "tests", "ml_plan_main.cpp"), *(os.path.join(csrc, f) for f in ("tuning.cpp", "ml_plan.cpp", "dist_plan.cpp"))]
    objs = [str(d / (os.path.basename(u) + ".o")) for u in units]
    jobs = [subprocess.Popen([*cxx, "-c", u, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for u, o in zip(units, objs)]
    for j in jobs:                                   # the four units compile side by side; any warning fails the build
        out = j.communicate()[0]
        assert j.returncode == 0 and not out.strip(), out
    r = subprocess.run([*cxx, *STATIC_RUNTIME, *objs, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    return exe


@pytest.mark.parametrize("grid,refine,k33,geo", PLAN_CASES)
def test_plan_under_sanitizers(grid, refine, k33, geo, sanitized_planner, recorded_plans, tmp_path):
    p, blk, ci, cj = _plan_input(grid, refine, k33)
    got = _sanitized_plan(sanitized_planner, tmp_path, p, blk, ci, cj, geo, 200, {})
    assert got == recorded_plans[_case_name(grid, geo)]


def _sanitized_plan(exe, tmp_path, p, blk, ci, cj, geo, coarsest_rows, knobs_env):
    """rows and hashes as plan_sha256 gives them, from the stand-alone program under the defaults plus knobs_env"""
    path = str(tmp_path / "matrix.bin")
    with open(path, "wb") as f:
        np.array([p.rowptr.size - 1, p.colind.size, blk.size - 1, int(geo)], np.int64).tofile(f)
        for a, dt in ((p.rowptr, np.int32), (p.colind, np.int32), (p.nzval, np.float64), (blk, np.int32), (ci, np.int32), (cj, np.int32)):
            np.ascontiguousarray(a, dt).tofile(f)
    env = {k: v for k, v in os.environ.items() if not k.startswith("NKP_")}        # defaults, whatever the caller tunes
    env.update(knobs_env)
    r = subprocess.run([exe, path, str(coarsest_rows)], capture_output=True, text=True, env=env, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "runtime error" not in out and "AddressSanitizer" not in out, out
    got = {"rows": [], "sha256": {"rows": None, "cmap": [], "col_of": []}}
    for line in r.stdout.splitlines():
        key, *vals = line.split()
        if key == "levels":
            got["rows"] = [int(v) for v in vals]
        elif key == "rows":
            got["sha256"]["rows"] = vals[0]
        elif key in ("cmap", "col_of"):
            got["sha256"][key].append(vals[0])
    return got


# one case per branch of the aggregation that the recorded plans, all at the default knobs, do not reach
@pytest.mark.parametrize("case", ["pocket0", "pocket9", "tau0", "tau5", "huge_from0", "ties_none_seed3", "deep_12x10x75", "odd_31x27x9", "stall", "near_stall"])
def test_plan_options_under_sanitizers(case, sanitized_planner, tmp_path, monkeypatch):
    p, blk, ci, cj, _ = msc.problem(case)
    msc.setenv(case, monkeypatch)
    rows, cmaps, colofs = solver.ml_plan_host(p.rowptr, p.colind, p.nzval, blk, ci, cj, coarsest_rows=msc.coarsest_rows(case))
    want = {"rows": [int(r) for r in rows], "sha256": {"rows": _sha(rows, np.int64), "cmap": [_sha(c, np.int32) for c in cmaps],
                                                       "col_of": [_sha(c, np.int32) for c in colofs]}}
    knobs_env = {msc.KNOB_ENV[k]: repr(v) for k, v in msc.plan_knobs(case).items()}
    got = _sanitized_plan(sanitized_planner, tmp_path, p, blk, ci, cj, True, msc.coarsest_rows(case), knobs_env)
    assert got["rows"] == msc.CASES[case].rows
    assert got == want
