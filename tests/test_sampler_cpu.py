"""The host side of the device sampler, without a GPU: the restatement tests/sampler_ref.py checked against definitions, the
independence of the draws of different seeds (stated on the restatement, which tests/test_sampler_gpu.py holds the kernels to),
sampler.alias_table, and the seed arithmetic of DeviceLoader."""
import itertools

import numpy as np
import pytest

import dropmask
import sampler_ref as R

U32, U64 = np.uint32, np.uint64
BIG_V = 10 ** 12          # 4096 draws of two seeds share an id by chance with probability 4096^2 / 10^12 = 1.7e-5
N_DRAWS = 4096


# ---- restatement self-checks -----------------------------------------------------------------------------------------------
def _nth_allowed_bsearch(ex, u):
    """The kernel's route to the u-th allowed item (sampler.hip nth_allowed), transcribed: checked against the definition."""
    lo, hi = 0, len(ex)
    while lo < hi:
        mid = (lo + hi) >> 1
        if ex[mid] - mid >= u + 1:
            hi = mid
        else:
            lo = mid + 1
    return u + lo


def _check_bijection(excl, V):
    excl = np.asarray(sorted(excl), dtype=np.int64)
    k = V - len(excl)
    got = R.nth_allowed(excl, V, np.arange(1, k + 1))
    assert got.shape == (k,) and (np.diff(got) > 0).all()                                  # one-to-one, ascending
    assert sorted(got.tolist() + excl.tolist()) == list(range(1, V + 1))                   # onto the allowed ids, none excluded
    assert [_nth_allowed_bsearch(excl.tolist(), u) for u in range(1, k + 1)] == got.tolist()


def test_nth_allowed_is_a_bijection_exhaustive():
    for V in range(1, 13):
        for m in range(0, V):
            for excl in itertools.combinations(range(1, V + 1), m):
                _check_bijection(excl, V)


@pytest.mark.parametrize("V", [2, 13, 1000])
def test_nth_allowed_hand_cases(V):
    k = max(1, V // 3)
    cases = [[1], [V], list(range(1, k + 1)), list(range(V - k + 1, V + 1)), list(range(1, V + 1, 2)), list(range(2, V + 1, 2)),
             list(range(1, V)), list(range(2, V + 1)), [i for i in range(1, V + 1) if i != (V + 1) // 2]]
    for excl in cases:
        if len(excl) < V:
            _check_bijection(excl, V)
    assert R.nth_allowed([], BIG_V, np.array([1, BIG_V])).tolist() == [1, BIG_V]


def test_mulhi64_equals_python_integers():
    rng = np.random.default_rng(0)
    edge = [0, 1, 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63) - 1, 1 << 63, (1 << 64) - 1]
    r = np.array(edge + rng.integers(0, 1 << 64, size=500, dtype=U64).tolist(), dtype=U64)
    for g in edge[1:] + [BIG_V, 2_000_000, 1_995_000] + rng.integers(1, 1 << 64, size=20, dtype=U64).tolist():
        assert R.mulhi64(r, g).tolist() == [(int(x) * int(g)) >> 64 for x in r.tolist()]
    assert int(R.mulhi64(np.array([(1 << 64) - 1], dtype=U64), 7)[0]) == 6                 # u = mulhi + 1 stays in 1..range


def test_draws_are_a_function_of_seed_and_index_only():
    excl, off = np.array([2, 5, 6], dtype=np.int64), np.array([0, 3, 3], dtype=np.int64)
    a = R.uniform_negatives(excl, off, [0, 0, 0, 0], 8, 40, seed=77)
    b = R.uniform_negatives(excl, off, [0, 0], 16, 40, seed=77)
    assert a.reshape(-1).tolist() == b.reshape(-1).tolist()                                # draw i = row * n + column
    assert not set(a.reshape(-1).tolist()) & {2, 5, 6}
    c = R.uniform_negatives(excl, off, [1, 0, 1, 0], 8, 40, seed=77)
    assert c[1].tolist() == a[1].tolist() and c[3].tolist() == a[3].tolist()               # the row's user changes only that row
    assert a.tolist() == R.uniform_negatives(excl, off, [0, 0, 0, 0], 8, 40, seed=77 + (1 << 64)).tolist()   # a 64-bit seed
    keys = {R.draw_key(s) for s in list(range(2000)) + [(h << 32) + l for h in range(40) for l in range(40)]}
    assert len(keys) == 2000 + 1600 - 40                                                   # distinct seeds, distinct round keys


# ---- seed independence -----------------------------------------------------------------------------------------------------
def _old_draw32(seed, ctr):
    """The draw this project shipped before: the seed's low word entered as a bare XOR with the counter's low word."""
    seed, ctr = int(seed) & R.MASK64, np.asarray(ctr, dtype=U64)
    lo, hi = (ctr & U64(R.MASK32)).astype(U32), (ctr >> U64(32)).astype(U32)
    return dropmask.rg_hash((seed >> 32) ^ 0x9E3779B9, dropmask.rg_hash(seed & R.MASK32, lo) ^ hi)


def _uniform_ids(seed, draw=R.draw32):
    """Sorted ids of draws 0 .. 4095 of the uniform kernel at V = 10**12 without exclusions."""
    return np.sort(R.mulhi64(R.variate64(seed, np.arange(N_DRAWS), draw), BIG_V).astype(np.int64) + 1)


def _alias_ids(seed, draw=R.draw32):
    """The same for the alias kernel's counters: the first try of draws 0 .. 4095 (counters 128 i, 128 i + 1) as one 64-bit variate."""
    h0, h1 = R.alias_variates(seed, np.arange(N_DRAWS), 0, draw)
    return np.sort(R.mulhi64((h0.astype(U64) << U64(32)) | h1.astype(U64), BIG_V).astype(np.int64) + 1)


def _loader_seeds(world=2, per_rank=32):
    """The seeds the first `per_rank` batches of every rank's DeviceLoader hand to the kernels, recorded from the loader itself."""
    from recguru_amd import sampler
    n = world * per_rank
    dom = sampler.DeviceDomain([[1 + i] for i in range(n)], np.ones(n, np.int64), np.ones(n, np.int64) * 2, 1000, "cpu")
    dom.batch = lambda users, L_enc, L_dec, eos, n_neg, seed: seed
    return [s for r in range(world) for s in sampler.DeviceLoader(dom, 1, 4, 4, 1001, 8, seed=0, rank=r, world=world)]


def _seed_sets(extra=()):
    sets = [sorted(set([s, s ^ 1, s ^ 2, s + 2, s + 6, s ^ (1 << 31), s + (1 << 32)] + [f(s) for f in extra]))   # (0 ^ 2 == 0 + 2)
            for s in (0, 11, (5 << 20) + 7)]
    loader = _loader_seeds()
    assert len(set(loader)) == 64
    return sets + [loader]


def _assert_independent(ids_of, sets):
    for seeds in sets:
        ids = [ids_of(s) for s in seeds]
        for (sa, a), (sb, b) in itertools.combinations(zip(seeds, ids), 2):
            shared = np.intersect1d(a, b).size
            assert shared == 0, "seeds %d and %d share %d of %d drawn ids" % (sa, sb, shared, N_DRAWS)
            assert not np.array_equal(a, b)                                                # (implied; the defect's own signature)


def test_seeds_share_no_uniform_draw():
    _assert_independent(_uniform_ids, _seed_sets())


def test_seeds_share_no_alias_draw():
    # the alias counters of one try are 128 apart: seeds 128 apart were the permuted pairs there
    _assert_independent(_alias_ids, _seed_sets(extra=(lambda s: s ^ 128, lambda s: s + 256)))


def test_seed_check_fails_on_the_old_scheme():
    """The property the fix removed, kept as a statement about the old draw: seeds 0 and 2 (any even difference) gave the same
    4096 variates in another order, seeds s and s ^ 1 the same with their halves swapped -- so the check above can fail."""
    a, b = _uniform_ids(0, _old_draw32), _uniform_ids(2, _old_draw32)
    assert np.array_equal(a, b) and np.intersect1d(a, b).size == np.unique(a).size
    assert np.array_equal(_uniform_ids(1000, _old_draw32), _uniform_ids(1006, _old_draw32))
    assert np.array_equal(_alias_ids(0, _old_draw32), _alias_ids(128, _old_draw32))
    r0, r1 = R.variate64(10, np.arange(N_DRAWS), _old_draw32), R.variate64(11, np.arange(N_DRAWS), _old_draw32)
    assert np.array_equal(r0, (r1 << U64(32)) | (r1 >> U64(32)))
    with pytest.raises(AssertionError):
        _assert_independent(lambda s: _uniform_ids(s, _old_draw32), [[0, 2]])


# ---- alias_table -----------------------------------------------------------------------------------------------------------
def _weight_vectors():
    rng = np.random.default_rng(3)
    for n in (2, 3, 31, 1000):
        w = rng.random(n) + 1e-3
        yield "random", w
        z = w.copy()
        z[rng.random(n) < 0.4] = 0.0
        z[0], z[-1] = 0.0, 1.0                                                             # slot 0 is the zero-weight id of a domain
        yield "zeros", z
        d = w * 1e-6
        d[n // 2] = 1.0
        yield "dominant", d
        dz = z * 1e-9
        dz[-1] = 1e9
        yield "dominant+zeros", dz
        yield "equal", np.ones(n)
        yield "zipf^0.75", np.concatenate([[0.0], np.floor(n / 2 / np.arange(1, n)) ** 0.75])


@pytest.mark.parametrize("kind,w", [pytest.param(k, w, id="%s-%d" % (k, len(w))) for k, w in _weight_vectors()])
def test_alias_table_reconstructs_the_distribution(kind, w):
    """Mass of id j under the table = (prob[j] + sum over slots i aliased to j of (1 - prob[i])) / n, with the f32 prob the kernel
    compares with.  Within 1e-6 of p[j] (f32 rounding of prob: 6e-8 per slot, n slots, over n) and EXACTLY 0 for a zero-weight
    id.  (A zero-weight id cannot be left in the `small` stack with prob = 1: the loop keeps sum(q) over the unplaced slots equal
    to their count up to rounding, so slots left when `large` runs out all have q = 1 - O(n eps).)"""
    from recguru_amd import sampler
    p = w / w.sum()
    prob, alias = sampler.alias_table(p)
    n = len(p)
    assert prob.dtype == np.float32 and alias.dtype == np.int32 and prob.shape == alias.shape == (n,)
    assert (prob >= 0).all() and (prob <= 1).all() and (alias >= 0).all() and (alias < n).all()
    mass = prob.astype(np.float64)
    np.add.at(mass, alias.astype(np.int64), 1.0 - prob.astype(np.float64))
    mass /= n
    assert np.abs(mass - p).max() <= 1e-6
    assert (mass[p == 0] == 0).all()


# ---- DeviceLoader seed arithmetic ------------------------------------------------------------------------------------------
def test_batch_seeds_are_pairwise_distinct():
    from recguru_amd import sampler
    rng = np.random.default_rng(1)
    counters = sorted(set([0, 1, 2, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 22) - 1, 1 << 22, (1 << 28) - 1]
                          + rng.integers(0, 1 << 22, size=1000).tolist()))
    seen = {}
    for seed in range(4):
        for rank in range(8):
            for c in counters:
                s = sampler.batch_seed(seed, rank, c)
                assert 0 <= s < 1 << 64 and s not in seen, (seed, rank, c, seen.get(s))
                seen[s] = (seed, rank, c)
                assert (s >> 40, (s >> 28) & 0xFFF, s & ((1 << 28) - 1)) == (seed, rank, c)     # the fields decode: one-to-one on the domain
    old = lambda seed, rank, c: ((seed * 1000003 + rank) << 20) + c                        # the packing before: 20 bits of counter
    assert old(0, 0, 1 << 20) == old(0, 1, 0)
    assert sampler.batch_seed(0, 0, 1 << 20) != sampler.batch_seed(0, 1, 0)
    top = sampler.batch_seed((1 << 24) - 1, (1 << 12) - 1, (1 << 28) - 1)
    assert top == (1 << 64) - 1
    for bad in [(1 << 24, 0, 0), (0, 1 << 12, 0), (0, 0, 1 << 28), (-1, 0, 0), (0, -1, 0), (0, 0, -1)]:
        with pytest.raises(ValueError):
            sampler.batch_seed(*bad)


def test_device_loader_hands_out_batch_seed():
    from recguru_amd import sampler
    got = _loader_seeds(world=2, per_rank=32)
    assert got == [sampler.batch_seed(0, r, i) for r in range(2) for i in range(32)]
    n = 8
    dom = sampler.DeviceDomain([[1 + i] for i in range(n)], np.ones(n, np.int64), np.ones(n, np.int64) * 2, 1000, "cpu")
    dom.batch = lambda users, L_enc, L_dec, eos, n_neg, seed: seed
    ld = sampler.DeviceLoader(dom, 2, 4, 4, 1001, 8, seed=3, rank=1, world=2)
    assert list(ld) + list(ld) == [sampler.batch_seed(3, 1, c) for c in range(4)]          # the counter runs on over epochs
    with pytest.raises(ValueError):
        sampler.DeviceLoader(dom, 2, 4, 4, 1001, 8, seed=1 << 24)
