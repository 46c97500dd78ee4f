"""The kernel selection rule and the group tables of the lane-per-column band solves (csrc/col_plan.cpp: col_plan) run alone, from
the stand-alone program tests/col_plan_main.cpp built with the address and undefined-behaviour sanitizers.  No GPU needed: the
unit is plain C++ without the HIP runtime; the program links it and csrc/tuning.cpp (the built-in tuning) and nothing else.

What the plan is held against:
  the selection       expected_kernel of tests/colsolve_cases.py, on level 0 of every case of CASES_CYCLE and on the column
                      preconditioner of every case of CASES_JACOBI under every family of FAMILIES, and on the hand-worked levels
  the group tables    their definition, from the column lengths: every column in exactly one group of its colour, the padding,
                      the running factor offsets, the slots, the sort order
  the row blocks      check_row_blocks of tests/colsolve_cases.py: consecutive, within both limits, greedy-maximal"""
import os
import subprocess

import numpy as np
import pytest

import colsolve_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nk_ocn_tracer_jacobian_precond_amd", "csrc")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
# the sanitizer runtimes are linked into the program itself, so that it starts the same in whatever environment it inherits
STATIC_RUNTIME = ["-static-libasan", "-static-libubsan"]
COL_LANES, COL_STREAM, COL_LDSRES, COL_LDSPACK = range(4)          # enum ColFamily
BATCH_WAVE, BATCH_LDSPACK2, BATCH_LDSPACK4 = range(3)              # enum ColBatch
SCALARS = ("rc", "family", "maxl", "wpe", "nch", "early", "pipe_min", "batch4", "batch_other", "wave_columns", "wave_fused", "gw", "stream",
           "ldsres", "sorted", "ngrp", "fac_total", "rhs_slots", "lds_doubles", "gs_ok", "gs_lds_bytes")
SHORT_ROW = 9                  # entries per row of the synthetic operator: far below GS_NNZ, as expected_kernel assumes


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("col_plan_asan")
    probe = d / "probe.cpp"
    probe.write_text("int main () { return 0; }\n")
    if subprocess.run(["g++", "-fsanitize=address", *STATIC_RUNTIME, str(probe), "-o", str(d / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler cannot link -fsanitize=address")
    exe = str(d / "col_plan_main")
    cxx = ["g++", "-std=c++17", "-Wall", "-ffp-contract=off", *SANITIZE]
    units = [os.path.join(ROOT, "tests", "col_plan_main.cpp"), os.path.join(CSRC, "col_plan.cpp"), os.path.join(CSRC, "tuning.cpp")]
    objs = [str(d / (os.path.basename(u) + ".o")) for u in units]
    jobs = [subprocess.Popen([*cxx, "-c", u, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for u, o in zip(units, objs)]
    for j in jobs:                                   # any warning fails the build
        out = j.communicate()[0]
        assert j.returncode == 0 and not out.strip(), out
    r = subprocess.run([*cxx, *STATIC_RUNTIME, *objs, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr
    return exe, d


# ---------------------------------------------------------------- cases in, plans out
class Case:
    """One input of col_plan: a tuning dict on top of the built-in one, the band, and the columns of every range in layout order."""

    def __init__(self, tuning, f32, P, dropped, colour_lens, multilevel=True, rowptr=None, max_len=None):
        self.knobs = cc.FAMILIES[tuning] if isinstance(tuning, str) else tuning      # the program starts from nkp_builtin_tuning
        self.T = dict(cc.TUNING_DEFAULTS, **self.knobs)
        self.f32, self.P, self.dropped, self.multilevel = int(f32), P, int(dropped), multilevel
        self.lens = [np.asarray(l, np.int64) for l in colour_lens]
        every = np.concatenate(self.lens)
        self.max_len = int(every.max()) if max_len is None else max_len
        self.blk_start = np.concatenate([[0], np.cumsum(every)])
        self.ranges = np.concatenate([[0], np.cumsum([l.size for l in self.lens])])
        self.fused = multilevel and self.T["ml_fused"] != 0
        self.rowptr = rowptr if rowptr is not None else SHORT_ROW * np.arange(self.blk_start[-1] + 1) if self.fused else None

    def text(self):
        def row(name, v):
            return f"{name} {len(v)} " + " ".join(str(int(x)) for x in v)
        lines = [f"tune {k} {int(v)}" for k, v in sorted(self.knobs.items())]
        lines += [f"P {self.P}", f"dropped {self.dropped}", f"max_len {self.max_len}", f"f32 {self.f32}", f"multilevel {int(self.multilevel)}"]
        lines += [row("blk_start", self.blk_start), row("ranges", self.ranges)]
        if self.rowptr is not None:
            lines.append(row("rowptr", self.rowptr))
        return "\n".join(lines) + "\n"


def run_plans(program, cases, chunk=256):
    """The plans of the cases, in order; the program takes a chunk of case files per start."""
    exe, d = program
    paths = []
    for i, c in enumerate(cases):
        paths.append(str(d / f"case_{i}.txt"))
        with open(paths[-1], "w") as f:
            f.write(c.text())
    plans = []
    for a in range(0, len(paths), chunk):
        r = subprocess.run([exe, *paths[a:a + chunk]], capture_output=True, text=True, timeout=120)
        out = r.stdout + r.stderr
        assert r.returncode == 0 and "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
        for ln in r.stdout.splitlines():
            key, *w = ln.split()
            if key == "case":
                plans.append({})
            elif key in SCALARS:
                plans[-1][key] = int(w[0])
            else:
                plans[-1][key] = np.array([int(x) for x in w], np.int64)
    for p in paths:
        os.remove(p)
    assert len(plans) == len(cases) and all(pl["rc"] == 0 for pl in plans)
    return plans


def lane_kernel(pl, c):
    """The instantiation launch_colblock_apply_lanes takes for a launch of any size (col_pipe_min is 1 where it is set)."""
    ft = "f32" if c.f32 else "f64"
    assert (pl["wpe"] == 3) == (pl["maxl"] == 80) and pl["maxl"] in (64, 80, 128) and pl["nch"] in (4, 5)
    if pl["family"] == COL_LDSPACK:
        return ("ldspack", c.P, pl["nch"])
    if pl["family"] == COL_LDSRES:
        return ("ldsres", c.P, ft, pl["early"])
    if pl["family"] == COL_STREAM:
        return ("stream", c.P, pl["gw"], ft)
    assert pl["family"] == COL_LANES
    if pl["pipe_min"] > 0:
        assert pl["pipe_min"] == c.T["col_pipe_min"]
        return ("lanes_pipe", c.P)
    return ("lanes", c.P, pl["maxl"], ft)


def kernels(pl, c):
    """The instantiations that serve single right-hand sides: which of the level's paths the cycle takes (multilevel.h,
    mlcycle.hip, mltail.hip) on top of the plan's choice."""
    ft, rpl = "f32" if c.f32 else "f64", 1 if c.max_len <= 64 else 2
    if c.multilevel and c.T["ml_tail_rows"] > 0:
        return {("tail", c.P, ft)}
    if pl["wave_fused"]:
        return {("gs_wave", c.P, rpl, ft), ("wave", c.P, rpl, ft)}
    if pl["wave_columns"]:
        return {("wave", c.P, rpl, ft)}
    if c.fused and pl["gs_ok"]:
        return {("gs_fused", c.P, ft), lane_kernel(pl, c)}
    return {lane_kernel(pl, c)}


def batch_kernels(pl, c, K):
    rpl = 1 if c.max_len <= 64 else 2
    kind = pl["batch4"] if K % 4 == 0 else pl["batch_other"]
    if kind == BATCH_WAVE:
        return {("wave_batch", c.P, rpl)} | ({("gs_wave_batch", c.P, rpl)} if pl["wave_fused"] else set())
    return {("ldspack4" if kind == BATCH_LDSPACK4 else "ldspack2", c.P, pl["nch"])}


def check_against_expected(pl, c, e):
    for field in ("stream", "ldsres", "gw", "ngrp", "lds_doubles", "gs_ok", "wave_columns", "wave_fused"):
        assert pl[field] == e[field], (field, pl[field], e[field])
    assert (pl["lds_doubles"] * 8 > 48 * 1024) == e["lds_over_48k"]
    assert kernels(pl, c) == e["kernels"], (kernels(pl, c), e["kernels"])
    for K in (2, 4, 8):
        assert batch_kernels(pl, c, K) == e["batch"](K), (K, batch_kernels(pl, c, K), e["batch"](K))


# ---------------------------------------------------------------- the selection
def test_plan_agrees_with_expected_kernel_on_the_cycle_cases(program):
    todo = []
    for grid, band, km, f32 in cc.CASES_CYCLE:
        P, dropped, max_len, ncols, lens = cc.level0(grid, band, km)
        for family in cc.FAMILIES:
            todo.append((Case(family, f32, P, dropped, lens), cc.expected_kernel(family, f32, P, dropped, max_len, ncols, lens), (family, grid, band, km, f32)))
    assert len(todo) == len(cc.CASES_CYCLE) * len(cc.FAMILIES)
    seen = set()
    for pl, (c, e, what) in zip(run_plans(program, [t[0] for t in todo]), todo):
        try:
            check_against_expected(pl, c, e)
        except AssertionError as err:
            raise AssertionError(f"{what}: {err}") from None
        seen |= kernels(pl, c) | {k for K in (2, 4, 8) for k in batch_kernels(pl, c, K)}
    assert {k[0] for k in seen} >= {"wave", "gs_wave", "lanes", "lanes_pipe", "stream", "ldsres", "ldspack", "ldspack2", "ldspack4", "gs_fused", "tail", "wave_batch"}


def test_plan_agrees_with_expected_kernel_on_the_column_preconditioner(program):
    todo = []
    for grid, band, km in cc.CASES_JACOBI:
        p = cc.problem(grid, km, band)
        lens = [np.diff(np.asarray(p.col_start(), np.int64))]            # one range, the columns in their natural order
        P, dropped, max_len = cc.stored_band(band), int(band > cc.MAX_BAND), int(lens[0].max())
        for family in cc.FAMILIES:
            e = cc.expected_kernel(family, 0, P, dropped, max_len, lens[0].size, lens, multilevel=False)
            todo.append((Case(family, 0, P, dropped, lens, multilevel=False), e, (family, grid, band, km)))
    for pl, (c, e, what) in zip(run_plans(program, [t[0] for t in todo]), todo):
        try:
            check_against_expected(pl, c, e)
            assert len(e["kernels"]) == 1 and not pl["wave_columns"] and not pl["gs_ok"] and pl["gs_rb"].size == 0
        except AssertionError as err:
            raise AssertionError(f"{what}: {err}") from None


def test_plan_agrees_on_the_hand_worked_levels(program):
    """Every level of colsolve_cases.HAND_WORKED, as 33 + 34 columns (one range of 67 for the column preconditioner) of max_len
    rows each -- the bounds that decide lds_over_48k without column lengths hold for any lengths."""
    cases = []
    for family, f32, P, dropped, max_len, multilevel, field, want in cc.HAND_WORKED:
        lens = [np.full(33, max_len), np.full(34, max_len)] if multilevel else [np.full(cc.HAND_WORKED_NCOLS, max_len)]
        cases.append(Case(family, f32, P, dropped, lens, multilevel=multilevel))
    for pl, c, (family, f32, P, dropped, max_len, multilevel, field, want) in zip(run_plans(program, cases), cases, cc.HAND_WORKED):
        if isinstance(field, tuple):
            got = batch_kernels(pl, c, field[1])
        elif field == "kernels":
            got = kernels(pl, c)
        elif field == "lds_over_48k":
            got = pl["lds_doubles"] * 8 > 48 * 1024
        else:
            got = pl[field]
        assert got == want, (family, f32, P, dropped, max_len, field, got, want)
    got = run_plans(program, [Case("lanes8", 0, 2, 0, [np.full(33, 128), np.full(34, 128)])])[0]
    assert got["lds_doubles"] == 1024 + 32 + 2 + 5 * 128 * 8 and got["ngrp"] == 10


# ---------------------------------------------------------------- the group tables
TABLE_FAMILIES = ("packed_sorted", "packed_unsorted", "ldsres", "stream32", "lanes8", "lanes32")


def check_group_tables(pl, c):
    gw, ngrp, ndiag = pl["gw"], pl["ngrp"], 2 * c.P + 1
    every = np.concatenate(c.lens)
    bs = c.blk_start
    pad = cc.LDSRES_CH if pl["ldsres"] else 8
    first = pl["grp_first"]
    assert first[0] == 0 and first[-1] == ngrp and first.size == len(c.lens) + 1
    assert [a.size for a in (pl["grp_b0"], pl["grp_nb"], pl["grp_maxlen"], pl["grp_base"])] == [ngrp] * 4
    assert pl["grp_row0"].size == 2 * ngrp and pl["col_slot"].size == 2 * ngrp * gw
    assert pl["grp_cols"].size == (ngrp * gw if pl["sorted"] else 0)
    row0, rows = pl["grp_row0"][:ngrp], pl["grp_row0"][ngrp:]
    slot, length = pl["col_slot"][:ngrp * gw].reshape(ngrp, gw), pl["col_slot"][ngrp * gw:].reshape(ngrp, gw)
    base = 0
    for r in range(len(c.lens)):
        cols = np.arange(c.ranges[r], c.ranges[r + 1])
        assert first[r + 1] - first[r] == (cols.size + gw - 1) // gw                       # grp_first brackets the colours
        members = []
        for g in range(first[r], first[r + 1]):
            nb = pl["grp_nb"][g]
            assert 1 <= nb <= gw and (nb == gw or g == first[r + 1] - 1)                    # only a colour's last group is partial
            mine = pl["grp_cols"][g * gw:g * gw + nb] if pl["sorted"] else pl["grp_b0"][g] + np.arange(nb)
            assert pl["grp_b0"][g] == mine[0]
            members.extend(mine)
            assert pl["grp_maxlen"][g] == (every[mine].max() + pad - 1) // pad * pad         # the longest member, padded
            assert pl["grp_base"][g] == base                                                # running sum of (2P+1) maxlen gw
            base += ndiag * pl["grp_maxlen"][g] * gw
            if pl["sorted"]:
                assert row0[g] == 0 and rows[g] == 0                                        # slots are absolute first rows
                assert (pl["grp_cols"][g * gw + nb:(g + 1) * gw] == -1).all()
            else:
                assert row0[g] == bs[mine[0]] and rows[g] == every[mine].sum()
            assert (slot[g, :nb] == bs[mine] - row0[g]).all() and (length[g, :nb] == every[mine]).all()
            assert not slot[g, nb:].any() and not length[g, nb:].any()                      # lanes beyond a partial group
        # every column of the colour in exactly one of its groups, and none of the other colour's
        assert sorted(members) == list(cols)
        if pl["sorted"]:
            # non-increasing chunk counts, ties in natural order: the stable sort of the natural order by chunk count
            ch = -((every[cols] + cc.LDSRES_CH - 1) // cc.LDSRES_CH)
            assert members == list(cols[np.argsort(ch, kind="stable")])
        else:
            assert members == list(cols)
    assert pl["fac_total"] == base
    assert c.rowptr is not None or (pl["gs_rb"].size == 0 and pl["gs_rb_ptr"].size == 0 and not pl["gs_ok"])


def test_group_tables(program):
    cases = []
    for grid in (cc.GRID_BIG, cc.GRID_SMALL):
        for km in (60, 80, 128):
            P, dropped, _, _, lens = cc.level0(grid, 2, km)
            cases += [Case(family, 1, P, dropped, lens) for family in TABLE_FAMILIES]
    plans = run_plans(program, cases)
    for pl, c in zip(plans, cases):
        check_group_tables(pl, c)
    # both orders and both paddings were there, and the sort moved columns
    assert {(pl["sorted"], pl["ldsres"]) for pl in plans} == {(1, 2), (0, 2), (0, 1), (0, 0)}
    assert any(pl["sorted"] and (pl["grp_cols"][:pl["grp_nb"][0]] != np.arange(pl["grp_nb"][0])).any() for pl in plans)
    assert any((pl["grp_nb"] < pl["gw"]).any() for pl in plans)


# ---------------------------------------------------------------- row blocks of the fused sweep
def check_plan_row_blocks(pl, c):
    ngrp = pl["ngrp"]
    ptr, rb = pl["gs_rb_ptr"], pl["gs_rb"]
    assert ptr.size == ngrp + 1 and ptr[0] == 0 and ptr[-1] == rb.size - 1 and rb[-1] == c.blk_start[-1]
    for g in range(ngrp):
        r0, r1 = pl["grp_row0"][g], pl["grp_row0"][g] + pl["grp_row0"][ngrp + g]
        assert rb[ptr[g + 1]] == r1                                              # the next group's first block begins where this one ends
        cc.check_row_blocks(c.rowptr, r0, r1, rb[ptr[g]:ptr[g + 1]])


def test_row_blocks_of_the_fused_sweep(program):
    P, dropped, _, _, lens = cc.level0(cc.GRID_BIG, 2, 128)
    n = int(sum(l.sum() for l in lens))
    rng = np.random.default_rng(11)
    rowptrs = {
        "rows bind": 3 * np.arange(n + 1),                                                  # GS_THREADS rows are 768 entries
        "entries bind": np.concatenate([[0], np.cumsum(rng.integers(5, 60, n))]),           # GS_NNZ entries are ~64 rows
        "a full row": np.concatenate([[0], np.cumsum(np.where(np.arange(n) % 97 == 5, cc.GS_NNZ, 7))]),   # a row of exactly GS_NNZ entries stands alone
    }
    cases = [Case(family, f32, P, dropped, lens, rowptr=rp) for rp in rowptrs.values() for family in ("gs_fused_lanes8", "gs_fused_stream32", "gs_fused_ldsres")
             for f32 in (0, 1)]
    plans = run_plans(program, cases)
    for pl, c in zip(plans, cases):
        check_plan_row_blocks(pl, c)
        check_group_tables(pl, c)
        fac = (2 * P + 1) * int(pl["grp_maxlen"].max()) * pl["gw"]
        assert pl["gs_lds_bytes"] == 8 * (cc.GS_NNZ + pl["rhs_slots"] + ((fac + 1) // 2 if c.f32 else fac))
        assert pl["gs_ok"] == int(pl["gs_lds_bytes"] <= 64 * 1024)
    assert {pl["gs_ok"] for pl in plans} == {0, 1}
    sizes = [np.diff(pl["gs_rb"]) for pl in plans]
    assert any((s == cc.GS_THREADS).any() for s in sizes) and any((s == 1).any() for s in sizes)
    # a row above GS_NNZ: no fused sweep, whatever else holds
    long_row = np.concatenate([[0], np.cumsum(np.where(np.arange(n) == n // 2, cc.GS_NNZ + 1, SHORT_ROW))])
    short = SHORT_ROW * np.arange(n + 1)
    with_long, without = run_plans(program, [Case("gs_fused_lanes8", 1, P, dropped, lens, rowptr=long_row), Case("gs_fused_lanes8", 1, P, dropped, lens, rowptr=short)])
    assert without["gs_ok"] == 1 and with_long["gs_ok"] == 0 and with_long["gs_rb"].size == 0 and with_long["gs_lds_bytes"] == 0
    for field in ("family", "gw", "ngrp", "lds_doubles", "rhs_slots", "fac_total"):
        assert with_long[field] == without[field]
