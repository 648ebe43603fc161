"""The large-array Blast link (csrc/pipeline_mimo_large.hip: mcle_run_mimo_large): cases shared by test_mimo_large_cpu.py (CPU:
the conditions on the inputs, the operand maps) and test_gpu_mimo_large.py (GPU: the kernels).  Every case is
oracle.chains.chain_mimo_scheme(scheme='blast') over realizations helpers.FLAT_FIRST .. FLAT_FIRST + FLAT_COUNT - 1 (3 .. 72) of
helpers.SEED with 16-QAM, computed once through helpers.flat_reference and shared read-only."""
from helpers import flat_reference

# (nt, nr, mmse, snr_db, columns): K-step padding (5 x 6, 7 x 9, 6 x 16), a partly filled row of 16 lanes (every nr < 16), stream
# counts that are no multiple of 4, column counts on each side of the 16- and 32-column tiles, an odd column count (51)
CASES = [(8, 8, False, 30.0, 130), (8, 8, True, 14.0, 130), (8, 16, False, 8.0, 130), (5, 6, False, 20.0, 51),
         (6, 16, True, 6.0, 51), (1, 16, False, -4.0, 130), (7, 9, False, 18.0, 34)]
CASE_IDS = ["%dx%d-%s-%gdB-%d" % (nt, nr, "mmse" if mmse else "zf", snr, ns) for nt, nr, mmse, snr, ns in CASES]

EDGE_SHAPES = [(8, 8), (5, 6)]
EDGE_COLUMNS = (1, 2, 15, 16, 17, 31, 32, 33, 51, 130)
EDGE_SNR = 16.0

FLAT_SHAPES = [(2, 2), (3, 4), (4, 4), (1, 3)]         # inside the envelope of mcle_run_mimo_flat too
FLAT_SNR, FLAT_NS = 16.0, 51

FORM_SHAPES = [(8, 8), (5, 6)]
FORM_COLUMNS = (51, 130)


def reference(nt, nr, mmse, snr, ns, mod="qam", M=16):
    return flat_reference("blast", mod, M, nt, nr, ns, snr, mmse, False)
