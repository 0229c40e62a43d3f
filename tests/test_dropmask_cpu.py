"""The host restatement of the dropout-mask contract (tests/dropmask.py) on its own: threshold rounding, keep fractions per
hash bit and per 16-bit half, independence of neighbouring words and of the seeds the dropout stream hands out one after
another, and the index spaces (distinct below the 32-bit wrap, and exactly where the attention map of config 5 wraps)."""
import numpy as np
import pytest

import dropmask as dm

N_WORDS = 1 << 18


def _words(seed, n=N_WORDS, start=0):
    return dm.rg_hash(dm.make_drop(0.3, seed).seed, np.arange(start, start + n, dtype=np.uint64).astype(np.uint32))


def _bits(w):
    return ((w[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & np.uint32(1)).astype(np.float64)


def test_make_drop_fields():
    for p, thresh in [(0.1, 6554), (0.2, 13107), (0.3, 19661), (0.5, 32768), (0.0, 0)]:
        c = dm.make_drop(p, 1)
        assert c.thresh == thresh, (p, c.thresh)
        assert c.onebit == (p == 0.5)
        if p > 0:
            assert c.inv_keep == float(np.float32(1) / (np.float32(1) - np.float32(p)))
    # the fold: a known value (the low half multiplied, the high half multiplied and offset, then a murmur-style finalizer)
    s = (0x1234 * 0x9E3779B1) & 0xFFFFFFFF ^ ((0x5 * 0x85EBCA77 + 0x165667B1) & 0xFFFFFFFF)
    s ^= s >> 15
    s = (s * 0x2C1B3C6D) & 0xFFFFFFFF
    s ^= s >> 12
    assert dm.make_drop(0.5, (0x5 << 32) | 0x1234).seed == s


def test_rg_hash_known_values():
    # rg_hash restated once more with Python integers
    def h(seed, x):
        x ^= seed
        x ^= x >> 16
        x = (x * 0x21F0AAAD) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x735A2D97) & 0xFFFFFFFF
        x ^= x >> 15
        return x
    xs = np.array([0, 1, 2, 31, 0x7FFFFFFF, 0xFFFFFFFF, 123456789], dtype=np.uint32)
    for seed in (0, 1, 0xDEADBEEF):
        assert [int(v) for v in dm.rg_hash(seed, xs)] == [h(seed, int(x)) for x in xs]


@pytest.mark.parametrize("p", [0.1, 0.2, 0.3, 0.5])
def test_keep_fraction_per_bit_and_per_half(p):
    c = dm.make_drop(p, (7 << 32) | 11)
    w = dm.rg_hash(c.seed, np.arange(N_WORDS, dtype=np.uint32))
    if c.onebit:        # one bit per element: every bit position keeps half of its elements
        frac = _bits(w).mean(0)
        sig = 0.5 / np.sqrt(N_WORDS)
        assert np.all(np.abs(frac - 0.5) < 5 * sig), frac
        idx = np.arange(32 * 4096, dtype=np.uint32)
        k = dm.keep_bool(c, idx).reshape(4096, 32)
        assert np.array_equal(k, _bits(w[:4096]).astype(bool))       # element 32 w + j = bit j of word w
    else:               # 16-bit mode: each half is compared with round(p * 65536)
        for half in (w & np.uint32(0xFFFF), w >> np.uint32(16)):
            drop = float((half < c.thresh).mean())
            sig = np.sqrt(p * (1 - p) / N_WORDS)
            assert abs(drop - c.thresh / 65536) < 5 * sig, (drop, p)
        idx = np.arange(2 * 4096, dtype=np.uint32)
        k = dm.keep_bool(c, idx).reshape(4096, 2)
        assert np.array_equal(k[:, 0], (w[:4096] & np.uint32(0xFFFF)) >= c.thresh)
        assert np.array_equal(k[:, 1], (w[:4096] >> np.uint32(16)) >= c.thresh)
    m = dm.keep(c.seed, p, np.arange(1 << 16, dtype=np.uint32))   # keep() takes the call seed, not the folded one
    assert set(np.unique(m)) <= {0.0, c.inv_keep}


def _agreement(a, b):
    """Mean fraction of equal bits of two word arrays and its worst bit position."""
    eq = 1.0 - _bits(a ^ b)
    return float(eq.mean()), float(np.abs(eq.mean(0) - 0.5).max())


def test_neighbouring_words_uncorrelated():
    w = _words(99)
    sig = 0.5 / np.sqrt(N_WORDS)
    mean, worst = _agreement(w[:-1], w[1:])
    assert abs(mean - 0.5) < 5 * sig / np.sqrt(32) + 1e-4 and worst < 5 * sig, (mean, worst)
    # the two 16-bit halves of a word (elements 2i and 2i+1 in the 16-bit mode)
    lo, hi = (w & np.uint32(0xFFFF)).astype(np.float64), (w >> np.uint32(16)).astype(np.float64)
    assert abs(np.corrcoef(lo, hi)[0, 1]) < 5 / np.sqrt(N_WORDS)


def test_successive_stream_seeds_uncorrelated():
    """ops._draw() hands out base << 32 | ctr: consecutive draws differ in the low half only, and two ranks' streams (or two
    manual seeds) at the same counter differ in the HIGH half only -- make_drop must fold both halves in."""
    from recguru_amd import ops
    seeds, saved = [], dict(ops._SEED)
    try:
        for s, rank in ((5, 0), (5, 1), (6, 0)):
            ops.manual_seed(s, rank)
            seeds.append([ops._draw() for _ in range(4)])
    finally:
        ops._SEED.update(saved)                                   # the process's dropout stream is left as it was found
    assert all(x >> 32 == seeds[0][0] >> 32 for x in seeds[0])
    assert len({x & 0xFFFFFFFF for row in seeds for x in row}) == 4          # only the high half tells the streams apart
    flat = [x for row in seeds for x in row]
    folded = {dm.make_drop(0.5, x).seed for x in flat}
    assert len(folded) == len(flat)
    sig = 0.5 / np.sqrt(N_WORDS)
    pairs = [(seeds[0][i], seeds[0][i + 1]) for i in range(3)] + [(seeds[0][i], seeds[1][i]) for i in range(4)] + \
            [(seeds[0][i], seeds[2][i]) for i in range(4)]
    for a, b in pairs:
        mean, worst = _agreement(_words(a), _words(b))
        assert abs(mean - 0.5) < 5 * sig and worst < 6 * sig, (hex(a), hex(b), mean, worst)


def test_rowmajor_index_distinct_below_the_wrap():
    r, c = np.meshgrid(np.arange(300), np.arange(257), indexing="ij")
    idx = dm.rowmajor_index(r, c, 257)
    assert idx.dtype == np.uint32 and len(np.unique(idx)) == idx.size
    assert np.array_equal(idx.astype(np.int64), r * 257 + c)
    # the index is 32 bits: row * ncols past 2^32 wraps
    assert int(dm.rowmajor_index(1 << 23, 0, 512)) == 0
    assert int(dm.rowmajor_index((1 << 23) - 1, 511, 512)) == 0xFFFFFFFF


@pytest.mark.parametrize("B,H,L", [(3, 2, 12), (2, 4, 50), (2, 1, 64), (1, 3, 100), (2, 2, 416)])
def test_attn_index_distinct_and_padded(B, H, L):
    b, h, q, k = np.meshgrid(np.arange(B), np.arange(H), np.arange(L), np.arange(L), indexing="ij")
    idx = dm.attn_index(b, h, q, k, H, L)
    assert len(np.unique(idx)) == idx.size
    lp = dm.lpad(L)
    assert lp % 32 == 0 and L <= lp < L + 32
    assert np.array_equal(idx.astype(np.int64), ((b * H + h) * L + q) * lp + k)
    assert np.all(idx[..., 0] % 32 == 0)                     # every query row starts on a hash-word boundary


def test_attn_index_wrap_at_config5():
    """Config 5 (BASELINE.json: B = 4096, H = 8, L = 400, LPAD = 416): B*H*L*LPAD = 5.45e9 > 2^32.  The first element past the
    wrap is key 256 of query 40 of head 3 of sequence 3226 (head index 25811); from sequence 3227 on every element is past it."""
    H, L = 8, 400
    assert dm.lpad(L) == 416 and 4096 * H * L * 416 > 1 << 32
    assert dm.attn_true_index(3226, 3, 40, 255, H, L) == (1 << 32) - 1
    assert int(dm.attn_index(3226, 3, 40, 255, H, L)) == 0xFFFFFFFF
    assert int(dm.attn_index(3226, 3, 40, 256, H, L)) == 0
    assert dm.attn_true_index(3227, 0, 0, 0, H, L) >= 1 << 32
    assert dm.attn_true_index(3226, 7, L - 1, L - 1, H, L) >= 1 << 32 > dm.attn_true_index(3226, 3, 40, 255, H, L)
    # below the wrap the index is the true one; past it the mask repeats an earlier sequence's (a known limit of the contract)
    assert int(dm.attn_index(3227, 0, 0, 0, H, L)) == dm.attn_true_index(3227, 0, 0, 0, H, L) - (1 << 32)
    # the hash WORD of an element is the word of the 32-bit index: true word mod 2^27
    tw = dm.attn_true_index(3300, 5, 7, 64, H, L) >> 5
    assert int(dm.attn_index(3300, 5, 7, 64, H, L)) >> 5 == tw % (1 << 27) != tw
    m = dm.attn_mask(1234, 0.5, H, L, [3300])
    assert m.shape == (1, H, L, L)
