"""On-device batch assembly and negative sampler against the host restatement of seq_padding
(synthetic.pad_sequences, itself pinned to the reference's seq_padding by tests/test_abi_and_host.py) and against the
distributional contract of pickle_loader.__getitem__ (uniform / freq^0.75 over 1..V minus the user's exclusions); and, id for
id, against the numpy restatement of the kernels (tests/sampler_ref.py): those comparisons are exact, none takes a tolerance."""
import itertools

import numpy as np
import pytest
import torch

import sampler_ref as R

pytestmark = pytest.mark.gpu


def _users(rng, n, V, Lmax):
    seqs = [rng.integers(1, V + 1, size=int(rng.integers(0, Lmax))).tolist() for _ in range(n)]
    seqs[0] = []                                            # empty user
    seqs[1] = rng.integers(1, V + 1, size=3 * Lmax).tolist()   # longer than any window
    val = rng.integers(1, V + 1, size=n)
    test = rng.integers(1, V + 1, size=n)
    return seqs, val, test


@pytest.mark.parametrize("L_enc,L_dec", [(12, 12), (16, 9), (3, 3), (2, 2), (1, 1)])
def test_assemble_batch_equals_seq_padding(L_enc, L_dec):
    from recguru_amd import sampler
    rng = np.random.default_rng(L_enc * 31 + L_dec)
    V = 97
    seqs, val, test = _users(rng, 23, V, 20)
    dom = sampler.DeviceDomain(seqs, val, test, V, "cuda")
    users = torch.as_tensor(rng.permutation(23))
    (enc, dec_in, dec_out), _, v, t = dom.batch(users, L_enc, L_dec, V + 1, 4, seed=1)
    for row, u in enumerate(users.tolist()):                # the reference's list arithmetic (data_loader.py:25-36)
        s = list(seqs[u])
        e = (s[-L_enc + 1:] if L_enc > 1 else []) + [V + 1] if len(s) >= L_enc else [0] * (L_enc - len(s) - 1) + s + [V + 1]
        di = ([0, 0] + e[0:-2])[-L_dec:]
        do = ([0, 0] + e[1:-1])[-L_dec:]
        assert enc[row].tolist() == e
        assert dec_in[row].tolist() == di
        assert dec_out[row].tolist() == do
    assert v.tolist() == val[users.numpy()].tolist() and t.tolist() == test[users.numpy()].tolist()


@pytest.mark.parametrize("exclude_val", [False, True])
def test_uniform_negatives(exclude_val):
    from recguru_amd import sampler
    rng = np.random.default_rng(5)
    V, n_users, n = 40, 6, 200000
    seqs, val, test = _users(rng, n_users, V, 12)
    dom = sampler.DeviceDomain(seqs, val, test, V, "cuda", exclude_val=exclude_val)
    users = torch.arange(n_users)
    _, neg, _, _ = dom.batch(users, 8, 8, V + 1, n, seed=11)
    _, neg2, _, _ = dom.batch(users, 8, 8, V + 1, n, seed=11)
    _, neg3, _, _ = dom.batch(users, 8, 8, V + 1, n, seed=12)
    assert torch.equal(neg, neg2) and not torch.equal(neg, neg3)           # counter-based: same seed, same draws
    neg = neg.cpu().numpy()
    assert neg.min() >= 1 and neg.max() <= V
    for u in range(n_users):
        own = set(seqs[u]) | {int(test[u])} | ({int(val[u])} if exclude_val else set())
        allowed = np.array([i for i in range(1, V + 1) if i not in own])
        cnt = np.bincount(neg[u], minlength=V + 1)
        assert cnt[[i for i in own if 1 <= i <= V]].sum() == 0             # never an excluded item
        if not exclude_val and int(val[u]) not in own:
            assert cnt[int(val[u])] > 0                                    # Q14: the validation item IS sampleable
        exp = n / len(allowed)
        chi2 = ((cnt[allowed] - exp) ** 2 / exp).sum()
        assert chi2 < len(allowed) + 6 * np.sqrt(2 * len(allowed))         # uniform over the allowed items


def test_weighted_negatives():
    from recguru_amd import sampler
    rng = np.random.default_rng(9)
    V, n = 30, 400000
    seqs, val, test = _users(rng, 3, V, 6)
    wf = np.concatenate([[0.0], rng.integers(1, 50, size=V).astype(np.float64)])
    dom = sampler.DeviceDomain(seqs, val, test, V, "cuda", wf=wf)
    _, neg, _, _ = dom.batch(torch.arange(3), 8, 8, V + 1, n, seed=3)
    neg = neg.cpu().numpy()
    p = np.power(wf, 0.75)
    for u in range(3):
        own = set(seqs[u]) | {int(test[u])}
        w = p.copy()
        w[list(own)] = 0
        w /= w.sum()
        cnt = np.bincount(neg[u], minlength=V + 1)
        assert cnt[list(own)].sum() == 0 and cnt[0] == 0
        live = w > 0
        chi2 = ((cnt[live] - n * w[live]) ** 2 / (n * w[live])).sum()
        assert chi2 < live.sum() + 6 * np.sqrt(2 * live.sum())


def test_device_loader_shards_and_shapes():
    from recguru_amd import sampler
    rng = np.random.default_rng(2)
    V = 200
    seqs, val, test = _users(rng, 64, V, 30)
    dom = sampler.DeviceDomain(seqs, val, test, V, "cuda")
    seen = []
    for rank in range(2):
        ld = sampler.DeviceLoader(dom, 8, 16, 16, V + 1, 16 * 3, seed=0, shuffle=True, rank=rank, world=2)
        assert len(ld) == 4
        for (enc, di, do), neg, v, t in ld:
            assert enc.shape == (8, 16) and neg.shape == (8, 48) and enc[:, -1].eq(V + 1).all()
            seen.append(t)
    assert torch.cat(seen).numel() == 64


def test_eval_loader_matches_test_seq_gen():
    """DeviceEvalLoader inputs == the reference's test_seq_gen list arithmetic (data_loader.py:39-55)."""
    from recguru_amd import sampler
    rng = np.random.default_rng(4)
    V, n, Le, Ld, C = 150, 16, 12, 12, 20
    seqs, val, test = _users(rng, n, V, 20)
    ld = sampler.DeviceEvalLoader(seqs, val, test, V, "cuda", 8, Le, Ld, V + 1, C)
    row = 0
    for (e_enc, e_dec, e_t), (t_enc, t_dec, t_t), nf, nr in ld:
        for i in range(e_enc.shape[0]):
            s, sv = list(seqs[row]), list(seqs[row]) + [int(val[row])]
            def pad(q):
                return q[-Le + 1:] + [V + 1] if len(q) >= Le else [0] * (Le - len(q) - 1) + q + [V + 1]
            ee, te = pad(s), pad(sv)
            assert e_enc[i].tolist() == ee and e_dec[i].tolist() == ([0] + ee[0:-1])[-Ld:]
            assert t_enc[i].tolist() == te and t_dec[i].tolist() == ([0] + te[0:-1])[-Ld:]
            assert int(e_t[i]) == int(val[row]) and int(t_t[i]) == int(test[row])
            own = set(s) | {int(val[row]), int(test[row])}
            assert not (set(nr[i].tolist()) & own) and nr.shape[1] == C
            row += 1
    assert row == 16


# ----------------------------------------------------------------------------------------------------------------------
# the kernels against their restatement (tests/sampler_ref.py): exact integer equality
# ----------------------------------------------------------------------------------------------------------------------
HI_SEED = (0x1234567 << 32) | 0x89ABCDEF                     # a seed whose high word is not zero


def _csr(sets):
    """Exclusion sets -> (excl, excl_off) int64 numpy, each set sorted and unique as DeviceDomain builds them."""
    sets = [np.unique(np.asarray(x, dtype=np.int64)) for x in sets]
    off = np.zeros(len(sets) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in sets], out=off[1:])
    return (np.concatenate(sets) if sets else np.zeros(0, np.int64)), off


def _draw(excl, off, users, n, V, seed, alias=None):
    from recguru_amd import hip
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    al = None if alias is None else (t(alias[0]), t(alias[1]))
    return hip.sample_negatives(t(excl), t(off), t(np.asarray(users, dtype=np.int64)), n, V, seed, al).cpu().numpy()


def test_uniform_negatives_equal_restatement_at_catalogue_scale():
    """V = 2 M, every shape of exclusion set, 16 rows of 70 000 draws: 1.12 M draws, more than the 4096 * 256 threads of the
    capped grid, so the grid-stride pass is compared as well."""
    rng = np.random.default_rng(21)
    V, n = 2_000_000, 70_000
    only = 1_234_567
    sets = [[], [1], [V], rng.choice(np.arange(1, V + 1), size=5000, replace=False), np.arange(1, 5001), np.arange(V - 4999, V + 1),
            np.setdiff1d(np.arange(1, V + 1), [only]), rng.choice(np.arange(1, V + 1), size=5000, replace=False)]
    excl, off = _csr(sets)
    users = [6, 3, 0, 5, 1, 7, 2, 4, 3, 6, 0, 0, 5, 2, 1, 4]                               # repeated and permuted
    got = _draw(excl, off, users, n, V, HI_SEED)
    exp = R.uniform_negatives(excl, off, users, n, V, HI_SEED)
    assert got.shape == (16, n) and got.dtype == np.int64
    assert np.array_equal(got, exp)
    assert (got[[0, 9]] == only).all()                                                     # V - 1 exclusions: one allowed id
    assert got.min() >= 1 and got.max() <= V
    for row, u in enumerate(users):
        assert not np.isin(got[row], sets[u]).any()
    assert (got[4] >= 2).all() and (got[6] < V).all() and (got[7] > 5000).all() and (got[3] <= V - 5000).all()


@pytest.mark.parametrize("seed", [0, 11, HI_SEED, (1 << 64) - 1])
def test_uniform_negatives_equal_restatement_smallest_shapes(seed):
    for sets, users, n, V in [([[]], [0], 1, 1), ([[]], [0, 0, 0], 5, 1), ([[1], [2], []], [0, 1, 2, 1], 7, 2), ([[2]], [0], 1, 2),
                              ([[3, 9], [], [1, 2, 3, 4, 5, 6, 7, 8, 9]], [2, 0, 1, 0, 2], 257, 10), ([[]], [0], 3, 10 ** 12)]:
        excl, off = _csr(sets)
        got = _draw(excl, off, users, n, V, seed)
        assert np.array_equal(got, R.uniform_negatives(excl, off, users, n, V, seed)), (sets, users, n, V)
        assert got.shape == (len(users), n) and got.min() >= 1 and got.max() <= V


def _zipf_domain():
    """V = 200 000, frequency floor(100 000 / id): ids above 100 000 have frequency 0.  The last user excludes ids 1..99 600 --
    all but (1 - 0.996^0.25) = 0.1 % of the freq^0.75 mass -- so 0.999^64 = 94 % of its draws reject 64 times and fall back."""
    from recguru_amd import sampler
    rng = np.random.default_rng(8)
    V = 200_000
    wf = np.concatenate([[0.0], np.floor(100_000 / np.arange(1, V + 1))])
    w = np.power(wf, 0.75)
    w[0] = 0.0                                                                             # DeviceDomain's table (data_loader.py:251-254)
    table = sampler.alias_table(w / w.sum())
    sets = [[], rng.choice(np.arange(1, V + 1), size=300, replace=False), np.arange(1, 2001), np.arange(1, 99_601)]
    return V, wf, table, sets


def test_alias_negatives_equal_restatement():
    from recguru_amd import sampler
    rng = np.random.default_rng(9)
    V = 30                                                                                 # the table of test_weighted_negatives: 31 slots
    wf = np.concatenate([[0.0], rng.integers(1, 50, size=V).astype(np.float64)])
    w = np.power(wf, 0.75)
    table = sampler.alias_table(w / w.sum())
    sets = [[], [1], [V], [3, 4, 5, 17], list(range(1, V))]
    excl, off = _csr(sets)
    users = [4, 0, 3, 1, 2, 0, 4]
    for seed, n in [(3, 5000), (HI_SEED, 1), (HI_SEED, 333)]:
        got = _draw(excl, off, users, n, V, seed, table)
        assert np.array_equal(got, R.alias_negatives(table[0], table[1], excl, off, users, n, V, seed))
        assert got.min() >= 1 and got.max() <= V and (got[[0, 6]] == V).all()
        for row, u in enumerate(users):
            assert not np.isin(got[row], sets[u]).any()


def test_alias_negatives_equal_restatement_zipf_and_fallback():
    """The 64-rejection fall-back is uniform over the allowed ids: it returns zero-frequency items, which torch.multinomial over
    the weights never would.  That is the stated behaviour (recguru_amd/sampler.py docstring); this test pins it."""
    V, wf, table, sets = _zipf_domain()
    excl, off = _csr(sets)
    users, n, seed = [3, 0, 1, 2, 3, 0], 4099, HI_SEED + 5
    got = _draw(excl, off, users, n, V, seed, table)
    exp, fell = R.alias_negatives(table[0], table[1], excl, off, users, n, V, seed, return_fallback=True)
    assert np.array_equal(got, exp)
    assert got.min() >= 1 and got.max() <= V
    for row, u in enumerate(users):
        assert not np.isin(got[row], sets[u]).any()
    assert fell[[0, 4]].mean() > 0.5 and not fell[[1, 2, 3, 5]].any()                      # most draws of the starved user fall back
    assert (wf[got[[1, 2, 3, 5]]] > 0).all()                                               # an accepted draw never has frequency 0 ...
    assert (wf[got[0][~fell[0]]] > 0).all() and (wf[got[0][fell[0]]] == 0).any()           # ... a fall-back draw can


def test_seeds_share_no_draw_on_the_device():
    """The pairwise check of tests/test_sampler_cpu.py through the kernel: 4096 draws at V = 10**12 without exclusions share an
    id by chance with probability 1.7e-5 per pair of seeds.  The draws of seeds an even amount apart used to be permutations of
    each other, those of s and s ^ 1 the same variates with their halves swapped."""
    V, n = 10 ** 12, 4096
    excl, off = _csr([[]])
    for a, b in [(0, 2), (11, 13), ((5 << 20) + 7, (5 << 20) + 9), (11, 10), (HI_SEED, HI_SEED + (1 << 32))]:
        ia, ib = _draw(excl, off, [0], n, V, a)[0], _draw(excl, off, [0], n, V, b)[0]
        assert np.intersect1d(ia, ib).size == 0, "seeds %d and %d share %d of %d ids" % (a, b, np.intersect1d(ia, ib).size, n)
        assert not np.array_equal(np.sort(ia), np.sort(ib))
        assert np.array_equal(ia, R.uniform_negatives(excl, off, [0], n, V, a)[0])
        assert np.array_equal(ib, R.uniform_negatives(excl, off, [0], n, V, b)[0])


def test_assemble_batch_equals_restatement_beyond_one_grid_pass():
    """B = 4096, L_enc = 200: 2.46 M output elements, past the 4096 * 256 threads of the capped grid; users empty, of length
    L_enc - 1, L_enc, L_enc + 1 and far longer; ids and eos above 2**31; L_dec == L_enc and L_dec < L_enc."""
    from recguru_amd import hip
    rng = np.random.default_rng(31)
    Le, B, eos = 200, 4096, (1 << 33) + 5
    lens = [0, 1, 2, Le - 2, Le - 1, Le, Le + 1, 3 * Le, 5000] + rng.integers(0, 2 * Le, size=91).tolist()
    seqs = [rng.integers(1, 1 << 40, size=k).tolist() for k in lens]
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    items = np.concatenate([np.asarray(s, dtype=np.int64) for s in seqs])
    users = np.concatenate([np.arange(len(seqs)), rng.integers(0, len(seqs), size=B - len(seqs))])
    users = users[rng.permutation(B)]
    t = lambda a: torch.as_tensor(a).cuda()
    for Ld in (Le, 137, 1):
        got = hip.assemble_batch(t(items), t(off), t(users), Le, Ld, eos)
        exp = R.assemble(seqs, users, Le, Ld, eos)
        for g, e, name in zip(got, exp, ("enc_in", "dec_in", "dec_out")):
            assert g.shape == e.shape and np.array_equal(g.cpu().numpy(), e), (name, Ld)


@pytest.mark.parametrize("world", [1, 2, 4])
def test_device_loader_epoch(world):
    """One epoch over all ranks: every user at most once, world * nb * bs of them, a rank's users congruent to its rank; a second
    epoch in another order; shuffle=False in the identity order; no id shared between the negatives of any two batches."""
    from recguru_amd import sampler
    rng = np.random.default_rng(2)
    V, n_users, bs, n_neg = 10 ** 12, 70, 8, 512
    seqs = [rng.integers(1, V + 1, size=int(k)).tolist() for k in rng.integers(0, 20, size=n_users)]
    val, test = np.arange(n_users) + 1000, rng.integers(1, V + 1, size=n_users)            # val[u] names the user of a row
    dom = sampler.DeviceDomain(seqs, val, test, V, "cuda")
    nb = (n_users // world) // bs
    seen, negs = [], []
    for rank in range(world):
        ld = sampler.DeviceLoader(dom, bs, 16, 16, V + 1, n_neg, seed=1, shuffle=True, rank=rank, world=world)
        assert len(ld) == nb
        epochs = []
        for _ in range(2):
            order = []
            for (enc, di, do), neg, v, t in ld:
                u = (v - 1000).cpu().numpy()
                assert neg.shape == (bs, n_neg) and (u % world == rank).all()
                assert np.array_equal(t.cpu().numpy(), test[u])
                e_enc, e_di, e_do = R.assemble(seqs, u, 16, 16, V + 1)
                assert np.array_equal(enc.cpu().numpy(), e_enc) and np.array_equal(di.cpu().numpy(), e_di)
                assert np.array_equal(do.cpu().numpy(), e_do)
                order.append(u)
                negs.append(neg.cpu().numpy().reshape(-1))
            epochs.append(np.concatenate(order))
        assert not np.array_equal(epochs[0], epochs[1])                                    # reshuffled
        seen.append(epochs[0])
        plain = sampler.DeviceLoader(dom, bs, 16, 16, V + 1, 4, seed=1, shuffle=False, rank=rank, world=world)
        got = np.concatenate([(v - 1000).cpu().numpy() for _, _, v, _ in plain])
        assert np.array_equal(got, np.arange(rank, n_users, world)[:n_users // world][:nb * bs])
    seen = np.concatenate(seen)
    assert seen.size == world * nb * bs == np.unique(seen).size
    for a, b in itertools.combinations(negs, 2):                                           # all batches of both epochs of all ranks
        assert np.intersect1d(a, b).size == 0


def test_eval_loader_negatives_equal_restatement_and_drop_last():
    """n_items_r / n_items_f are the uniform / alias draws under seeds 2 s / 2 s + 1, s = (seed << 20) + epoch * nb + batch; 20
    users at batch 8 give 2 batches of 8 (the reference's DataLoader(drop_last=True)): the last 4 users are not scored."""
    from recguru_amd import sampler
    rng = np.random.default_rng(4)
    V, n, C, seed = 150, 20, 20, 3
    seqs, val, test = _users(rng, n, V, 20)
    wf = np.concatenate([[0.0], rng.integers(0, 50, size=V).astype(np.float64)])
    ld = sampler.DeviceEvalLoader(seqs, val, test, V, "cuda", 8, 12, 12, V + 1, C, wf=wf, seed=seed)
    d = ld.eval_dom
    excl, off = d.excl.cpu().numpy(), d.excl_off.cpu().numpy()
    prob, al = d.alias[0].cpu().numpy(), d.alias[1].cpu().numpy()
    for epoch in range(2):
        batches = list(ld)
        assert len(ld) == 2 and [b[0][0].shape[0] for b in batches] == [8, 8]
        for i, (ev, te, n_f, n_r) in enumerate(batches):
            u = np.arange(8 * i, 8 * i + 8)
            s = (seed << 20) + epoch * 2 + i
            assert np.array_equal(ev[2].cpu().numpy(), val[u]) and np.array_equal(te[2].cpu().numpy(), test[u])
            assert np.array_equal(n_r.cpu().numpy(), R.uniform_negatives(excl, off, u, C, V, 2 * s))
            assert np.array_equal(n_f.cpu().numpy(), R.alias_negatives(prob, al, excl, off, u, C, V, 2 * s + 1))
