"""CPU: the reference-signal sequences and the NumPy restatement of the channel estimators against the reference's own
numbers (tests/golden/g1_chanest.npz, written by scripts/make_golden_chanest.py)."""
import importlib.util
import os

import numpy as np
import pytest

import chanest_oracle as co
from helpers import GOLDEN
from pyphysim_amd import reference_signals as rs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "g1_chanest.npz"), allow_pickle=False)


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_chanest",
                                                  os.path.join(REPO, "scripts", "make_golden_chanest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _close(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float(np.max(np.abs(a - b))) <= TOL


def test_sequences_equal_the_reference(gold):
    _close(rs.calcBaseZC(139, 25), gold["seq_zc139_u25"])
    root = rs.RootSequence(root_index=25, size=150)
    assert (root.size, root.Nzc, root.index) == (150, 149, 25)
    _close(root.seq_array(), gold["seq_root150_u25"])
    far = rs.RootSequence(root_index=7, size=75, Nzc=31)            # extension past twice the length
    assert (far.size, far.Nzc) == (75, 31)
    _close(far.seq_array(), gold["seq_root75_nzc31_u7"])
    _close(rs.SrsUeSequence(root, 0).seq_array(), gold["seq_srs150_cs0"])
    _close(rs.SrsUeSequence(root, 7).seq_array(), gold["seq_srs150_cs7"])
    _close(rs.get_srs_seq(root.seq_array(), 7), gold["seq_srs150_cs7"])
    dmrs = rs.DmrsUeSequence(root, 11, cover_code=np.array([1, -1]))
    assert dmrs.size == 150 and dmrs.seq_array().shape == (2, 150) and not dmrs.normalized
    assert np.array_equal(dmrs.cover_code, [1, -1])
    _close(dmrs.seq_array(), gold["seq_dmrs150_cs11_occ"])
    norm = rs.SrsUeSequence(rs.RootSequence(root_index=25, Nzc=139), 3, normalize=True)
    assert norm.normalized and norm.size == 139 and abs(np.linalg.norm(norm.seq_array()) - 1) < 1e-14
    _close(norm.seq_array(), gold["seq_srs139_cs3_norm"])


def test_extension_and_primes():
    assert np.array_equal(rs.get_extended_ZF(np.array([1, 2, 3, 4, 5]), 8), [1, 2, 3, 4, 5, 1, 2, 3])
    assert np.array_equal(rs.get_extended_ZF(np.array([1, 2, 3]), 10), [1, 2, 3, 1, 2, 3, 1, 2, 3, 1])
    assert [rs.largest_prime_not_above(n) for n in (2, 3, 36, 37, 150, 300, 1200, 2048)] == [2, 3, 31, 37, 149, 293, 1193,
                                                                                            2039]


def test_error_types():
    with pytest.raises(ValueError, match="phi"):
        rs.RootSequence(root_index=3, size=12)
    with pytest.raises(ValueError):
        rs.RootSequence(root_index=3, size=24)
    with pytest.raises(AttributeError):
        rs.RootSequence(root_index=3)
    with pytest.raises(AttributeError):
        rs.RootSequence(root_index=3, size=40, Nzc=41)
    with pytest.raises(AssertionError):
        rs.get_srs_seq(np.ones(4, dtype=complex), 8)


def test_restatement_equals_the_reference(gold):
    gen = _generator()
    for name, (ne, u, ncs, K, m, rows, norm) in gen.EST_CASES.items():
        ref, rx, want = (gold["est_%s_%s" % (name, k)] for k in ("ref", "rx", "out"))
        _close(co.estimate(ref, rx, K, m, norm), want)
        _close(co.estimate_pruned(ref, rx, K, m, norm), want)
    K = gen.OCC_CASE[3]
    _close(co.estimate_occ(gold["occ_ref"], [1, -1], gold["occ_rx"], K), gold["occ_out"])
    _close(co.estimate_occ(gold["occ_ref"], [1, -1], gold["occ_rx"], K), gold["occ_out_flat"])
    _close(co.estimate_occ(gold["occ_ref"], [1, -1], gold["occ_rx"][0], K), gold["occ_out_1ant"])


def test_product_sequences_match_the_fixture_inputs(gold):
    """The sequences the GPU tests estimate with are the ones this package builds."""
    gen = _generator()
    for name, (ne, u, ncs, K, m, rows, norm) in gen.EST_CASES.items():
        ue = rs.SrsUeSequence(rs.RootSequence(root_index=u, size=ne), ncs, normalize=norm)      # (2048: our sieve finds 2039)
        _close(ue.seq_array(), gold["est_%s_ref" % name])


def test_realization_restatement_recovers_orthogonal_users_exactly():
    """Without noise, users whose taps fall outside each other's window are recovered to rounding."""
    root = rs.RootSequence(root_index=7, size=48)
    cfg = dict(ref_seqs=np.stack([rs.SrsUeSequence(root, s).seq_array() for s in (0, 2, 5)]), n_rx=2, size_multiplier=2,
               num_taps_to_keep=5, noise_var=0.0, tap_power=[1.0, 0.5, 0.25, 0.125], tap_delay=[0, 1, 2, 4])
    for r in range(4):
        err, pw = co.chanest_realization(11, r, cfg)
        assert np.all(err / pw < 1e-26)


def test_generator_reproduces_the_fixture(gold):
    """Array for array: the sequences, the seeded received arrays and the estimator's sequences bit for bit; the estimator
    outputs, which pass through two FFTs whose kernels NumPy picks by the host's vector extensions, to 1e-12."""
    gen = _generator()
    if not os.path.isdir(os.path.join(gen.REF, "pyphysim", "reference_signals")):
        pytest.skip("no reference checkout at %s" % gen.REF)
    made = gen.build_fixture()
    assert sorted(made) == sorted(gold.files)
    for k in gold.files:
        assert made[k].dtype == gold[k].dtype and made[k].shape == gold[k].shape, k
        if "_out" in k:
            _close(made[k], gold[k])
        else:
            assert np.array_equal(made[k], gold[k]), k
