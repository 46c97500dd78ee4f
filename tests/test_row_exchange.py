"""RowExchange (csrc/row_exchange.h), the one type behind every exchange of rows of a row-distributed solver, alone in the
stand-alone program tests/row_exchange_main.cpp built with the address and undefined-behaviour sanitizers: one row wide it hands
out the plan's own counts, K = 2, 4, 8 wide those counts times K -- also when the width narrows again on a live exchange (4, 2,
8, 1, 4), with no ranks at all and with ranks that exchange nothing -- and a copy on which drop_wide () was called (a batch
member) shares the one-row pointers, has no K-wide ones, scales on its own and leaves the original as it was."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "nk_ocn_tracer_jacobian_precond_amd", "csrc")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
STATIC_RUNTIME = ["-static-libasan", "-static-libubsan"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("row_exchange_asan")
    probe = d / "probe.cpp"
    probe.write_text("int main () { return 0; }\n")
    if subprocess.run(["g++", "-fsanitize=address", *STATIC_RUNTIME, str(probe), "-o", str(d / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler cannot link -fsanitize=address")
    exe = str(d / "row_exchange_main")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *SANITIZE, *STATIC_RUNTIME, "-I", CSRC, os.path.join(HERE, "row_exchange_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0 and not (r.stdout + r.stderr).strip(), r.stdout + r.stderr      # any warning fails the build
    return exe


def test_counts_at_every_width_and_copies_under_the_sanitizers(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=60)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "runtime error" not in out and "AddressSanitizer" not in out and "FAILED" not in out, out[-4000:]
    assert r.stdout.strip() == "ok", out[-4000:]

