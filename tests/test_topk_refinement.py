"""The bound refinement of csrc/topk.hip row_topk_kernel (round 6: 1024-bin radix histograms instead of bisecting the
64-bit key space), restated in numpy and run on the distributions that defeat a threshold taken from thread-local maxima:
all-equal scores (keys differ in the index bits only), heavy ties, a dense cluster just above the bound, huge dynamic
range, NaNs of every sign and payload (whose keys lie above +inf's).  Checks the loop's invariant and exit condition --
kk <= count(key >= T) <= capacity -- and that it terminates in a handful of passes, from the kernel's start hi = ~0; the
start before that (rank_key(row max, ~0)) is shown to break the invariant on NaN rows.  Also the ranking key itself: its
order is np.argsort(x, kind="stable")[::-1] on every float class.  The kernel is checked against np.argsort on the GPU
(tests/test_gpu_topk_exact.py, tests/test_gpu_parity.py test_topk_rows_exact).  Replaces np.argsort(...)[::-1] of reference src/hipporag/HippoRAG.py:1500,1688,1746
and torch.topk of utils/embed_utils.py:55,73 wherever only a prefix is read."""
import numpy as np
import pytest

CAP, BINS = 4096, 1024
ORDERED_NAN = 0xFFC00000            # csrc/common.h kOrderedNaN: every NaN, one value above +inf (0xff800000)
KEY_MAX = (1 << 64) - 1


def _ordered(f32):
    u = f32.view(np.uint32).astype(np.uint64)
    return np.where(u >> np.uint64(31), ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))


def _rank_order(x):
    """The upper 32 bits of csrc/common.h rank_key: f32_to_ordered(x + 0) (-0 folded into +0), every NaN -> ORDERED_NAN"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):                             # signalling NaNs
        return np.where(np.isnan(x), np.uint64(ORDERED_NAN), _ordered(x + np.float32(0)))


def _keys(scores):
    return (_rank_order(scores) << np.uint64(32)) | np.arange(len(scores), dtype=np.uint64)


def _old_hi(scores):
    """The refinement's start before the fix: rank_key(mx, ~0), mx = fmaxf over the row from -inf: NaN is skipped (an
    all-NaN row gives -inf)"""
    mx = np.fmax.reduce(np.concatenate([[-np.inf], scores]).astype(np.float32))
    return (int(_rank_order(np.array([mx]))[0]) << 32) | 0xFFFFFFFF


def _histogram(keys, lo, hi):
    """one pass of the loop: the bin shift and the suffix counts (keys in the bins >= b) of lo <= key <= hi"""
    width = hi - lo
    shift = 0
    while (width >> shift) >= BINS:
        shift += 1
    inside = keys[(keys >= np.uint64(lo)) & (keys <= np.uint64(hi))]
    hist = np.bincount(((inside - np.uint64(lo)) >> np.uint64(shift)).astype(np.int64), minlength=BINS)
    return shift, np.cumsum(hist[::-1])[::-1]


def _invariant(keys, kk, lo, hi, above):
    """count(key > hi) = above < kk <= above + count(lo <= key <= hi)"""
    in_range = int(((keys >= np.uint64(lo)) & (keys <= np.uint64(hi))).sum())
    return int((keys > np.uint64(hi)).sum()) == above and above < kk <= above + in_range


def refine(keys, kk, lo, hi=KEY_MAX):
    """-> (T, passes): the loop of row_topk_kernel's overflow path, one histogram pass per iteration; it starts at
    hi = ~0, above every key (NaN keys included)"""
    lo, above, passes = int(lo), 0, 0
    while True:
        passes += 1
        assert _invariant(keys, kk, lo, hi, above)
        shift, suffix = _histogram(keys, lo, hi)
        assert above < kk <= above + suffix[0]                      # bin 0 qualifies: the search below finds a bin
        b = int(np.flatnonzero(above + suffix >= kk).max())
        c_ge = above + int(suffix[b])
        c_gt = above + (int(suffix[b + 1]) if b + 1 < BINS else 0)
        blo = lo + (b << shift)
        if c_ge <= CAP or shift == 0:
            return blo, passes
        above, lo, hi = c_gt, blo, min(hi, blo + (1 << shift) - 1)


def _nan(sign, payload):
    return np.array([(sign << 31) | 0x7F800000 | payload], np.uint32).view(np.float32)[0]


NAN_PAYLOADS = [_nan(s, p) for s in (0, 1) for p in (0x400000, 0x1, 0x7FFFFF, 0x400001, 0x12345)]


@pytest.mark.parametrize("name", ["normal", "all_equal", "heavy_ties", "cluster_above_the_bound", "wide_range", "two_values"])
@pytest.mark.parametrize("kk", [1, 200, 2047, 2048])
def test_refinement_reaches_a_bound_that_fits(name, kk):
    rng = np.random.default_rng(len(name) + kk)
    n = 300_000
    s = {"normal": lambda: rng.standard_normal(n),
         "all_equal": lambda: np.full(n, 0.25),
         "heavy_ties": lambda: np.round(rng.standard_normal(n) * 4) / 4,
         "cluster_above_the_bound": lambda: np.where(rng.random(n) < 0.2, 0.5 + 1e-6 * rng.random(n), rng.random(n) * 0.4),
         "wide_range": lambda: rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n),
         "two_values": lambda: rng.choice([-1.0, 1.0], n)}[name]().astype(np.float32)
    keys = _keys(s)
    start = np.sort(keys)[max(0, n - 20000)]                        # a loose bound: 20 000 keys at or above it
    T, passes = refine(keys, kk, start)
    count = int((keys >= np.uint64(T)).sum())
    assert kk <= count <= CAP, (name, kk, count)
    assert passes <= 7                                              # 64 bits at 10 bits per pass
    want = np.sort(keys)[::-1][:kk]                                 # and the top-kk of the candidates are THE top-kk
    got = np.sort(keys[keys >= np.uint64(T)])[::-1][:kk]
    np.testing.assert_array_equal(got, want)


def _nan_row(name, rng, n):
    x = rng.standard_normal(n).astype(np.float32)
    pick = lambda m: rng.choice(n, m, replace=False)
    if name == "few_nans":
        x[pick(5)] = np.float32(np.nan)
    elif name == "more_nans_than_kk":
        x[pick(3000)] = np.float32(np.nan)
    elif name == "negative_and_mixed_payload_nans":
        at = pick(2500)
        x[at] = np.array(NAN_PAYLOADS, np.float32)[np.arange(len(at)) % len(NAN_PAYLOADS)]
    elif name == "all_nan":
        x[:] = _nan(1, 0x7FFFFF)
    elif name == "nan_and_infs":
        x[pick(1000)] = np.inf
        x[pick(1000)] = -np.inf
        x[pick(1500)] = np.array(NAN_PAYLOADS, np.float32)[0:1].repeat(1500)
    return x


@pytest.mark.parametrize("name", ["few_nans", "more_nans_than_kk", "negative_and_mixed_payload_nans", "all_nan",
                                  "nan_and_infs"])
@pytest.mark.parametrize("kk", [1, 200, 2047, 2048])
def test_refinement_with_nans(name, kk):
    rng = np.random.default_rng(len(name) * 7 + kk)
    n = 300_000
    keys = _keys(_nan_row(name, rng, n))
    start = np.sort(keys)[max(0, n - 20000)]
    T, passes = refine(keys, kk, start)
    count = int((keys >= np.uint64(T)).sum())
    assert kk <= count <= CAP, (name, kk, count)
    assert passes <= 7
    want = np.sort(keys)[::-1][:kk]
    np.testing.assert_array_equal(np.sort(keys[keys >= np.uint64(T)])[::-1][:kk], want)


@pytest.mark.parametrize("name", ["few_nans", "more_nans_than_kk", "all_nan"])
def test_old_start_breaks_the_invariant_on_nan_rows(name):
    """The start before the fix, hi = rank_key(fmaxf(row), ~0), lies below every NaN key: count(key > hi) is the number
    of NaNs, not 0 -- the loop's invariant is false from the first pass.  With more NaNs than kk no bin qualifies at all
    (the kernel then read a stale count as the bin index); the start hi = ~0 keeps the invariant on the same row."""
    rng = np.random.default_rng(11)
    n, kk = 300_000, 2047
    x = _nan_row(name, rng, n)
    keys = _keys(x)
    start = int(np.sort(keys)[n - 4500])                            # 4500 > CAP keys at or above it: the overflow path
    hi = _old_hi(x)
    assert not _invariant(keys, kk, start, hi, 0)
    assert int((keys > np.uint64(hi)).sum()) == int(np.isnan(x).sum())
    if name != "few_nans":                                          # >= 2453 of the 4500 are NaN: < kk keys in [lo, hi]
        _, suffix = _histogram(keys, start, hi)
        assert not np.any(suffix >= kk)                             # no bin qualifies
    assert _invariant(keys, kk, start, KEY_MAX, 0)
    T, _ = refine(keys, kk, start)
    np.testing.assert_array_equal(np.sort(keys[keys >= np.uint64(T)])[::-1][:kk], np.sort(keys)[::-1][:kk])


def _every_float_class(rng, n):
    """rows drawn from +-0, subnormals, +-FLT_MIN, +-FLT_MAX, +-inf, NaNs of both signs with several payloads, and
    ordinary values -- with many exact repeats"""
    fi = np.finfo(np.float32)
    sub = np.array([1, 2, 0x7FFFFF, 0x400000], np.uint32).view(np.float32)
    nans = np.array(NAN_PAYLOADS, np.float32)
    special = np.concatenate([np.array([0.0, -0.0], np.float32), sub, -sub,
                              np.array([fi.tiny, -fi.tiny, fi.max, -fi.max, np.inf, -np.inf], np.float32), nans,
                              np.array([1.0, -1.0, 0.5, np.nextafter(np.float32(1), np.float32(2))], np.float32)])
    x = rng.standard_normal(n).astype(np.float32)
    at = rng.random(n) < 0.6
    x[at] = special[rng.integers(0, len(special), int(at.sum()))]
    return x


@pytest.mark.parametrize("seed", range(4))
def test_rank_key_order_is_numpy_argsort(seed):
    """Sorting by the fixed rank_key (descending) is np.argsort(x, kind="stable")[::-1] exactly: every NaN above +inf
    whatever its sign or payload, ties (+0 / -0, repeated values, NaNs) broken by the larger index."""
    rng = np.random.default_rng(seed)
    x = _every_float_class(rng, 5000)
    keys = _keys(x)
    assert keys.min() > 0                                           # key 0 marks an empty slot, never an element
    got = np.argsort(keys)[::-1]                                    # keys are unique
    np.testing.assert_array_equal(got, np.argsort(x, kind="stable")[::-1])
    # the decoded score of a NaN key is the canonical quiet NaN
    nan_keys = _rank_order(x)[np.isnan(x)]
    assert np.all(nan_keys == ORDERED_NAN)
    assert np.uint32(ORDERED_NAN & 0x7FFFFFFF) == np.float32(np.nan).view(np.uint32)
