"""Config 4: the C++ kernel selection (csrc/c4_select.hpp::c4_select, the function mcle_run_mimo_ofdm launches from) against the
independent Python replay of tests/test_gpu_c4_edges.py (c4_tag), line by line over the whole cross product of shapes, arithmetics,
options and link cases.  scripts/c4_select_dump.cpp is the selection as a stand-alone program (host compiler, no HIP): it reads one
query per line and prints the tag of the plan, or "refused".

The one difference by design: the generic kernel at (2048, 4 x 4) in complex128 is refused by its LAUNCHER (168 KiB of LDS,
run_mimo_impl's MCLE_REQUIRE), not by the selection -- there c4_select names "mimo_ofdm_generic<2048,4> f64" and the replay, which
answers for the whole call, says refused."""
import itertools
import os
import subprocess

import pytest

from test_gpu_c4_edges import BOTH, LINKS, PAIRS, REFUSED, SIZES, THREADS, _cp, _used, c4_tag, dec_kind

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINK_CASES = ("in", "slicer", "cp0", "cp15", "band", "psk8", "nocert", "psk4", "qpsk")
MFMA_VARIANTS = (0, 36, 32, 30, 21)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("c4_select") / "c4_select_dump")
    subprocess.run(["c++", "-std=c++17", "-I", "include", "-I", "pyphysim_amd/csrc", "scripts/c4_select_dump.cpp", "-o", exe],
                   cwd=REPO, check=True)               # no host compiler: this fails, it does not skip
    return exe


def _queries():
    for n, (nt, nr), dt, thr, gen, nom, mf, lk in itertools.product(SIZES, PAIRS, BOTH, THREADS, (0, 1), (0, 1), (0, 1), LINK_CASES):
        for var in (MFMA_VARIANTS if mf else (0,)):
            yield n, nt, nr, dt, thr, gen, nom, mf, var, lk


def test_selection_agrees_with_the_replay_over_the_cross_product(dump):
    queries = list(_queries())
    assert len(queries) == 6 * 10 * 2 * len(THREADS) * 2 * 2 * (1 + len(MFMA_VARIANTS)) * len(LINK_CASES)
    lines = []
    for n, nt, nr, dt, thr, gen, nom, mf, var, lk in queries:
        link = LINKS[lk]
        lines.append("%d %d %d %d %d %d %d %d %d %d %d %d %d" % (dt == "f64", n, nt, nr, _used(link, n), _cp(link), link["M"], dec_kind(link),
                                                                 thr, gen, nom, mf, var))
    out = subprocess.run([dump], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[-1] == "" and len(out) == len(queries) + 1
    launcher_refusals = 0
    for got, (n, nt, nr, dt, thr, gen, nom, mf, var, lk) in zip(out, queries):
        want = c4_tag(n, nt, nr, dt, LINKS[lk], thr, gen, nom, mf, var)
        if got == "mimo_ofdm_generic<2048,4> f64":      # the launcher-side refusal: selected, then refused for its LDS
            assert want == REFUSED and (n, nt, nr, dt) == (2048, 4, 4, "f64"), (got, want, n, nt, nr, dt, thr, gen, nom, mf, var, lk)
            launcher_refusals += 1
            continue
        assert got == want, (got, want, n, nt, nr, dt, thr, gen, nom, mf, var, lk)
    print("queries %d, distinct tags %d, launcher-side refusals %d" % (len(queries), len(set(out)) - 2, launcher_refusals))
    assert launcher_refusals > 0


def test_a_short_query_is_an_error(dump):
    r = subprocess.run([dump], input="1 1024 4 4\n", capture_output=True, text=True)
    assert r.returncode == 2 and r.stdout == ""
