"""The one-launch half sweep's part of the column plan (csrc/col_plan.cpp: ColKernel::lane_fused, ColPlan::grp_tile) run alone, from
the stand-alone program tests/col_plan_lane_main.cpp built with the address and undefined-behaviour sanitizers like
tests/test_col_plan.py builds its program.  No GPU needed.

What the plan is held against:
  the selection    expected_lane_fused below: expected_kernel of tests/colsolve_cases.py extended by the rule of the new kernel --
                   packed layout, not one column per wave, a level of the cycle, columns of at most 64 rows, half bandwidth <= 2,
                   0 < columns <= ml_lane_fused -- on a qualifying level and on one level per way of not qualifying
  the tile map     its definition: per group slot the slot's column counted in columns that have rows, -1 for a slot without a
                   column and for a column without rows; absent (and ntile = 0) where lane_fused is 0"""
import os
import subprocess

import numpy as np
import pytest

import colsolve_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nk_ocn_tracer_jacobian_precond_amd", "csrc")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
STATIC_RUNTIME = ["-static-libasan", "-static-libubsan"]
COL_LDSPACK = 3
DEFAULT_LANE_FUSED = 50000
SCALARS = ("builtin_ml_lane_fused", "rc", "family", "nch", "wave_columns", "wave_fused", "lane_fused", "gw", "sorted", "ngrp", "ntile")
PACKED = dict(col_wave_max=0, col_ldsres_min=1)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("col_plan_lane_asan")
    probe = d / "probe.cpp"
    probe.write_text("int main () { return 0; }\n")
    if subprocess.run(["g++", "-fsanitize=address", *STATIC_RUNTIME, str(probe), "-o", str(d / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler cannot link -fsanitize=address")
    exe = str(d / "col_plan_lane_main")
    cxx = ["g++", "-std=c++17", "-Wall", "-ffp-contract=off", *SANITIZE]
    units = [os.path.join(ROOT, "tests", "col_plan_lane_main.cpp"), os.path.join(CSRC, "col_plan.cpp"), os.path.join(CSRC, "tuning.cpp")]
    r = subprocess.run([*cxx, *STATIC_RUNTIME, *units, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr        # any warning fails the build
    return exe, d


class Case:
    def __init__(self, tuning, colour_lens, f32=1, P=2, dropped=0, multilevel=True):
        self.knobs, self.f32, self.P, self.dropped, self.multilevel = tuning, int(f32), P, int(dropped), multilevel
        self.lens = [np.asarray(l, np.int64) for l in colour_lens]
        self.every = np.concatenate(self.lens)
        self.max_len = int(self.every.max())
        self.ncols = int(self.every.size)
        self.blk_start = np.concatenate([[0], np.cumsum(self.every)])
        self.ranges = np.concatenate([[0], np.cumsum([l.size for l in self.lens])])

    def text(self):
        def row(name, v):
            return f"{name} {len(v)} " + " ".join(str(int(x)) for x in v)
        lines = [f"tune {k} {int(v)}" for k, v in sorted(self.knobs.items())]
        lines += [f"P {self.P}", f"dropped {self.dropped}", f"max_len {self.max_len}", f"f32 {self.f32}", f"multilevel {int(self.multilevel)}"]
        return "\n".join(lines + [row("blk_start", self.blk_start), row("ranges", self.ranges)]) + "\n"


def run_plans(program, cases):
    exe, d = program
    paths = []
    for i, c in enumerate(cases):
        paths.append(str(d / f"case_{i}.txt"))
        with open(paths[-1], "w") as f:
            f.write(c.text())
    r = subprocess.run([exe, *paths], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
    plans = []
    for ln in r.stdout.splitlines():
        key, *w = ln.split()
        if key == "case":
            plans.append({})
        elif key in SCALARS:
            plans[-1][key] = int(w[0])
        else:
            plans[-1][key] = np.array([int(x) for x in w], np.int64)
    assert len(plans) == len(cases) and all(pl["rc"] == 0 for pl in plans)
    return plans


def expected_lane_fused(c):
    """expected_kernel of colsolve_cases.py, extended: lane_fused, and the instantiation the half sweeps of such a level take"""
    e = cc.expected_kernel(c.knobs, c.f32, c.P, c.dropped, c.max_len, c.ncols, c.lens, multilevel=c.multilevel)
    limit = c.knobs.get("ml_lane_fused", DEFAULT_LANE_FUSED)
    e["lane_fused"] = int(c.multilevel and e["ldsres"] == 2 and not e["wave_columns"] and c.max_len <= 64 and c.P <= 2 and 0 < c.ncols <= limit)
    if e["lane_fused"]:
        e["kernels"] = e["kernels"] | {("gs_lanes_diag", c.P, 4)}
    return e


def check(pl, c):
    e = expected_lane_fused(c)
    assert pl["builtin_ml_lane_fused"] == DEFAULT_LANE_FUSED
    for field in ("wave_columns", "wave_fused", "gw", "ngrp", "lane_fused"):
        assert pl[field] == e[field], (field, pl[field], e[field])
    assert (pl["family"] == COL_LDSPACK) == (e["ldsres"] == 2)
    assert (("gs_lanes_diag", c.P, pl["nch"]) in e["kernels"]) == bool(pl["lane_fused"])
    if not pl["lane_fused"]:
        assert pl["grp_tile"].size == 0 and pl["ntile"] == 0
        return e
    gw, ngrp = pl["gw"], pl["ngrp"]
    assert gw == 32 and pl["nch"] == 4 and pl["grp_tile"].size == ngrp * gw
    tile_of = np.where(c.every > 0, np.cumsum(c.every > 0) - 1, -1)
    assert pl["ntile"] == int((c.every > 0).sum())
    gt = pl["grp_tile"].reshape(ngrp, gw)
    for g in range(ngrp):
        nb = pl["grp_nb"][g]
        cols = pl["grp_cols"][g * gw:g * gw + nb] if pl["sorted"] else pl["grp_b0"][g] + np.arange(nb)
        assert (gt[g, :nb] == tile_of[cols]).all() and (gt[g, nb:] == -1).all()
    return e


def lens_two_colours(rng, n0, n1, top=64, low=1):
    a, b = rng.integers(low, top + 1, n0), rng.integers(low, top + 1, n1)
    a[0] = top                                   # the longest column decides max_len
    return [a, b]


def test_lane_fused_levels_and_their_tile_map(program):
    rng = np.random.default_rng(5)
    fused = dict(PACKED, ml_lane_fused=10 ** 6)
    cases = [
        Case(fused, lens_two_colours(rng, 40, 70)),                                   # several groups, partial last ones
        Case(dict(fused, col_sort_groups=0), lens_two_colours(rng, 40, 70)),          # groups of consecutive columns
        Case(fused, lens_two_colours(rng, 7, 32, top=20)),                            # one partial group, one full one; short columns
        Case(fused, lens_two_colours(rng, 33, 64, top=48), P=1),
        Case(fused, lens_two_colours(rng, 40, 70, low=0)),                            # columns without rows: no tile
        Case(dict(fused, col_sort_groups=0), lens_two_colours(rng, 40, 70, low=0)),
        Case(dict(PACKED, ml_lane_fused=110), lens_two_colours(rng, 40, 70)),         # exactly the limit
        Case(PACKED, lens_two_colours(rng, 40, 70)),                                  # the built-in limit
    ]
    plans = run_plans(program, cases)
    for pl, c in zip(plans, cases):
        e = check(pl, c)
        assert pl["lane_fused"] == 1 and e["ldsres"] == 2
    assert any((c.every == 0).any() for c in cases) and {pl["sorted"] for pl in plans} == {0, 1}
    assert any((pl["grp_tile"] != np.where(pl["grp_cols"] >= 0, pl["grp_cols"], -1)).any() for pl in plans if pl["sorted"])     # a tile that is not its column's number


def test_levels_that_do_not_qualify(program):
    rng = np.random.default_rng(6)
    fused = dict(PACKED, ml_lane_fused=10 ** 6)
    lens = lens_two_colours(rng, 40, 70)
    cases = {
        "65 rows": Case(fused, lens_two_colours(rng, 40, 70, top=65)),
        "P = 4": Case(fused, lens, P=4),
        "f64 factors": Case(fused, lens, f32=0),
        "not packed": Case(dict(fused, col_ldsres_packed=0), lens),
        "one column per wave": Case(dict(fused, col_wave_max=10 ** 6), lens),
        "switched off": Case(dict(fused, ml_lane_fused=0), lens),
        "one column too many": Case(dict(fused, ml_lane_fused=109), lens),
        "too few columns for the packed family": Case(dict(col_wave_max=0, ml_lane_fused=10 ** 6), lens),
        "column preconditioner": Case(fused, [np.concatenate(lens)], f32=0, multilevel=False),
        "tail kernel": Case(dict(fused, ml_tail_rows=16000), lens),
    }
    plans = run_plans(program, list(cases.values()))
    for (what, c), pl in zip(cases.items(), plans):
        try:
            check(pl, c)
            assert pl["lane_fused"] == 0
        except AssertionError as err:
            raise AssertionError(f"{what}: {err}") from None
