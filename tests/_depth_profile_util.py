"""Expected values of depth_profile (per window row and bin the positions shared with every build row of the window's contig,
summed) without the engine, and the cases its tests share.

A window covers L positions from S (Strict rows [start, end): L = end - start; Weak rows [start, end]: L = end - start + 1); its
bin edges in half-open position space are x_j = S + floor(j L / B), j = 0 .. B (L <= 0 reads as 0: every bin is empty).  The
expectation expands every window to its B bins as rows of an ordinary probe frame (``explicit_bins``) and takes
_depth_sum_util.prefix_form of that frame -- the form tests/test_depth_sum_cpu.py holds against the pair and block forms --
reshaped to (n, B), the flagged rows reversed."""
import numpy as np

import _depth_sum_util as S

I32_MIN, I32_MAX = S.I32_MIN, S.I32_MAX

# constants of the code under test that the cases are sized by (depth_profile.hip.h)
TILE = 256                       # DPROF_TILE: consecutive edges of one item across the workgroup's lanes (4 wavefronts of 64)
ITEMS = 4                        # DPROF_ITEMS: edges per thread
WG_SLOTS = TILE * ITEMS          # DPROF_WG_SLOTS: edges a workgroup evaluates
WG_EDGES = WG_SLOTS - 1          # DPROF_WG_EDGES: edges a workgroup advances by (its last edge is the next one's first)
MAX_BINS = 4096                  # DPROF_MAX_BINS
CM_LDS = S.CM_LDS


def edges(window, n_bins, strict):
    """the B + 1 bin edges of one window (start, end) in half-open position space, Python ints"""
    s, e = int(window[0]), int(window[1])
    length = max(e - s + (0 if strict else 1), 0)
    return [s + j * length // n_bins for j in range(n_bins + 1)]


def edges_np(ws, we, n_bins, strict):
    """the same for arrays of windows: int64 (n, B + 1); j L < 2^13 x 2^32 fits int64"""
    ws, we = np.asarray(ws).astype(np.int64), np.asarray(we).astype(np.int64)
    length = np.maximum(we - ws + (0 if strict else 1), 0)
    return ws[:, None] + length[:, None] * np.arange(n_bins + 1, dtype=np.int64)[None, :] // np.int64(n_bins)


def explicit_bins(windows, n_bins, strict):
    """the n x B bin frame, row i * B + j = bin j of window i, int64 columns in the windows' own convention (an empty bin comes
    out as a row that covers no position)"""
    wc, ws, we = (np.asarray(a).astype(np.int64) for a in windows)
    x = edges_np(ws, we, n_bins, strict)
    return np.repeat(wc, n_bins), x[:, :-1].reshape(-1), x[:, 1:].reshape(-1) - (0 if strict else 1)


def bin_lengths(windows, n_bins, strict, reverse=None):
    x = edges_np(windows[1], windows[2], n_bins, strict)
    return _reversed(np.diff(x, axis=1), reverse)


def _reversed(m, reverse):
    if reverse is not None:
        m = m.copy()
        rev = np.asarray(reverse, bool)
        m[rev] = m[rev, ::-1]
    return m


def expected_bases(windows, build, strict, n_contigs, n_bins, reverse=None):
    n = len(windows[0])
    flat = S.prefix_form(explicit_bins(windows, n_bins, strict), build, strict, n_contigs)
    return _reversed(flat.reshape(n, n_bins), reverse)


def assert_profile_equal(got, exp, what=""):
    got = np.asarray(got)
    assert got.dtype == np.int64 and got.shape == exp.shape, f"{what}: {got.dtype} {got.shape} != {exp.shape}"
    bad = np.argwhere(got != exp)
    assert bad.size == 0, f"{what}: {len(bad)} bins differ, first (row, bin) {tuple(bad[0])}: {got[tuple(bad[0])]} != {exp[tuple(bad[0])]}"


# ---- cases -------------------------------------------------------------------------------------------------------------------------

# build-side shapes of _depth_sum_util whose probes serve as windows
SHAPES = ["three_rows", "crowded_bins", "wide_grid", "contigs_cm_lds", "contigs_cm_lds_plus", "int32_limits", "int32_limits_inverted",
          "degenerate_build", "zero_length_build", "degenerate_probe", "touching_nested", "empty_probe", "empty_build",
          "one_sided_contigs"]
SHAPE_BINS = 5                   # odd and small: most windows of these shapes are longer, a few shorter (empty bins)

N_BINS = [1, 2, 63, 64, 65, 100, MAX_BINS]

# (rows, bins) with rows x (bins + 1) one less than, equal to and one more than the tile and the workgroup's advance / slots, and the
# same around two workgroups
BOUNDARIES = [(85, 2), (128, 1), (4, 63), (1, 256),                      # 255, 256, 256, 257 edges
              (14, 72), (341, 2), (93, 10), (16, 63), (512, 1), (25, 40), (205, 4),     # 1022, 1023, 1023, 1024, 1024, 1025, 1025
              (31, 65), (23, 88), (89, 22), (32, 63), (683, 2)]          # 2046 = 2 WG_EDGES, 2047, 2047, 2048, 2049
assert sorted({n * (b + 1) for n, b in BOUNDARIES}) == [TILE - 1, TILE, TILE + 1, WG_EDGES - 1, WG_EDGES, WG_SLOTS, WG_SLOTS + 1,
                                                        2 * WG_EDGES, 2 * WG_EDGES + 1, 2 * WG_SLOTS, 2 * WG_SLOTS + 1]


def small_build(seed=21, n=3000, n_contigs=2, span=60_000):
    rng = np.random.default_rng(seed)
    return S.U.random_rows(rng, n, n_contigs, span, 400), n_contigs


def random_windows(seed, n, n_contigs, span=60_000, max_len=5000):
    return S.U.random_rows(np.random.default_rng(seed), n, n_contigs, span, max_len)


def length_windows(n_bins, strict):
    """windows of L = 0, 1, B - 1, B, B + 1, two primes and a negative length, on both contigs of small_build, in the mode's convention"""
    lens = [0, 1, max(n_bins - 1, 0), n_bins, n_bins + 1, 7919, 104_729, -3]
    starts = [100, 20_000, 3, 40_000, 777, 10_000, -50_000, 500]
    ws = np.array(starts * 2, np.int64)
    we = ws + np.array(lens * 2, np.int64) - (0 if strict else 1)
    return S.as_i32(np.repeat([0, 1], len(lens)), ws, we)


def whole_range_windows(strict):
    """windows over all of int32 (L = 2^32 - 1 Strict, 2^32 Weak: j L needs 64 bits) and over its halves"""
    ws = np.array([I32_MIN, I32_MIN, 0, I32_MIN + 1, -1], np.int64)
    we = np.array([I32_MAX, 0, I32_MAX, I32_MAX - 1, I32_MAX], np.int64)
    return S.as_i32(np.array([0, 1, 2, 0, 1]), ws, we)


def mixed_flags(n, seed=5):
    return np.random.default_rng(seed).integers(0, 2, n).astype(bool)
