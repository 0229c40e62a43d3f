"""On-device batch assembly and negative sampling.

Replaces pickle_loader.__getitem__ + the DataLoader collation of the reference (GURU/data/data_loader.py:276-316,
455-483): a domain lives on the GPU as CSR item sequences plus, per user, the sorted exclusion set of the negative
sampler; a batch -- ((enc_in, dec_in, dec_out), n_items, val, test), the reference's layout -- is two kernel
launches (rg_assemble_batch, rg_sample_negatives) and FRESH negatives are drawn for every batch, as the reference
does per __getitem__ (the pre-staged TensorLoader keeps one static draw per user).

Quirk Q14: in the reference the loop `for val in seq: weights[seq] = 0` rebinds `val`, so the line
`weights[val] = 0` zeroes the last sequence item again and the held-out VALIDATION item stays sampleable; only the
sequence and the test item are excluded.  exclude_val=False (default) reproduces that, True excludes it as well.

The frequency-weighted draw (an alias table over freq^0.75) redraws while the candidate is excluded; a user whose exclusions
hold nearly all of the mass can fail all 64 tries, and the draw then FALLS BACK to the uniform draw over the user's allowed
items.  That fall-back can return a zero-frequency item, which torch.multinomial over the weights never would
(tests/test_sampler_gpu.py pins it as the stated behaviour).

Seeds: every launch takes a 64-bit seed, all of whose bits reach the draws (csrc/sampler.hip draw_key; tests/sampler_ref.py
restates the draws exactly).  DeviceLoader gives every (loader seed, rank, batch counter) a seed of its own -- batch_seed.
"""
import numpy as np
import torch

from . import hip


def alias_table(p):
    """Walker/Vose alias table of a probability vector (numpy float64) -> (prob f32, alias i32)."""
    p = np.asarray(p, dtype=np.float64)
    n = len(p)
    q = p * (n / p.sum())
    prob = np.ones(n, dtype=np.float64)
    alias = np.arange(n, dtype=np.int64)
    small = [i for i in range(n) if q[i] < 1.0]
    large = [i for i in range(n) if q[i] >= 1.0]
    while small and large:
        s, l = small.pop(), large.pop()
        prob[s], alias[s] = q[s], l
        q[l] = q[l] - (1.0 - q[s])
        (small if q[l] < 1.0 else large).append(l)
    return prob.astype(np.float32), alias.astype(np.int32)


SEED_BITS, RANK_BITS, COUNTER_BITS = 24, 12, 28


def batch_seed(seed, rank, counter):
    """The 64-bit sampler seed of batch `counter` (= epoch * batches per epoch + batch) of rank `rank` of a DeviceLoader built
    with `seed`: the three fields side by side, seed << 40 | rank << 28 | counter.  One-to-one on its domain
    0 <= seed < 2**24, 0 <= rank < 2**12, 0 <= counter < 2**28; outside it two loaders could share a seed, so that is an error."""
    seed, rank, counter = int(seed), int(rank), int(counter)
    if not (0 <= seed < 1 << SEED_BITS and 0 <= rank < 1 << RANK_BITS and 0 <= counter < 1 << COUNTER_BITS):
        raise ValueError("batch_seed: need 0 <= seed < 2**%d, 0 <= rank < 2**%d, 0 <= counter < 2**%d (got %d, %d, %d)"
                         % (SEED_BITS, RANK_BITS, COUNTER_BITS, seed, rank, counter))
    return (seed << (RANK_BITS + COUNTER_BITS)) | (rank << COUNTER_BITS) | counter


HARD_POOL_SEED = 0x5DEECE66D          # the hard-negative pool's draw: the batch seed with these bits flipped


class DeviceDomain(object):
    """One domain's users on the device: CSR sequences, exclusion sets, val / test items."""

    def __init__(self, seqs, val, test, V, device, exclude_val=False, wf=None):
        n = len(seqs)
        lens = np.fromiter((len(s) for s in seqs), dtype=np.int64, count=n)
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        items = np.concatenate([np.asarray(s, dtype=np.int64) for s in seqs]) if n else np.zeros(0, np.int64)
        ex, exoff = [], np.zeros(n + 1, dtype=np.int64)
        for i, s in enumerate(seqs):
            own = list(s) + [test[i]] + ([val[i]] if exclude_val else [])
            e = np.unique(np.asarray(own, dtype=np.int64))
            e = e[(e >= 1) & (e <= V)]
            if len(e) >= V:
                raise ValueError("user %d excludes the whole catalogue" % i)
            ex.append(e)
            exoff[i + 1] = exoff[i] + len(e)
        t = lambda a: torch.as_tensor(a).to(device)
        self.V, self.n, self.device = int(V), n, device
        self.items, self.offsets = t(items), t(off)
        exc = np.concatenate(ex) if n else np.zeros(0, np.int64)
        self.excl, self.excl_off = t(exc), t(exoff)
        self.val, self.test = t(np.asarray(val, dtype=np.int64)), t(np.asarray(test, dtype=np.int64))
        self.alias = None
        self._no_excl = None
        self._w = None                                       # the draw's weights (float64, host), kept for the logQ tables
        self._host_excl = (exc, exoff)
        self._logq = None
        self._inclusion = {}
        if wf is not None:                                   # data_loader.py:251-254
            w = np.power(np.asarray(wf, dtype=np.float64), 0.75)
            w[0] = 0.0
            prob, al = alias_table(w / w.sum())
            self.alias = (t(prob), t(al))
            self._w = w

    # ---- logQ correction of the sampled softmax: host tables in float64, built on first use ----
    def _q(self):
        """(Q, Qf) over the rows 0 .. V + 1 of the item table: Q the draw's distribution (w / sum w over 1..V, or 1 / V without
        frequencies; 0 at row 0, the EOS row and zero-frequency ids), Qf the same with every zero of 1..V raised to the smallest
        positive Q -- such ids can be labels and the sampler's uniform fall-back can draw them, and a bias has to be finite."""
        V = self.V
        Q = np.zeros(V + 2, dtype=np.float64)
        if self._w is None:
            Q[1:V + 1] = 1.0 / V
        else:
            m = min(len(self._w), V + 1)
            Q[1:m] = self._w[1:m]
            Q /= Q.sum()
        Qf = Q.copy()
        body = Qf[1:V + 1]
        body[body <= 0.0] = body[body > 0.0].min()
        return Q, Qf

    def logq_tables(self):
        """(neg_bias [V + 2] f32, m_u [users] f64 host, pos_shift [users] f32): -log Qf per table row (0 at row 0 and the EOS row);
        each user's exclusion mass m_u = sum of Q over its exclusion row; and -log(1 - m_u), the part of pos_bias that does not
        depend on k (1 - m_u no smaller than the smallest positive Q, so that it stays finite)."""
        if self._logq is None:
            Q, Qf = self._q()
            V = self.V
            nb = np.zeros(V + 2, dtype=np.float64)
            nb[1:V + 1] = -np.log(Qf[1:V + 1])
            exc, exoff = self._host_excl
            run = np.concatenate([np.zeros(1), np.cumsum(Q[exc])])
            m_u = run[exoff[1:]] - run[exoff[:-1]]
            shift = -np.log(np.maximum(1.0 - m_u, Qf[1:V + 1].min()))
            t = lambda a: torch.as_tensor(a.astype(np.float32)).to(self.device)
            self._logq = (t(nb), m_u, t(shift))
        return self._logq

    def inclusion_bias(self, n):
        """[V + 2] f32, cached per n: -log of the probability that a row is among n independent draws from Qf,
        -log(1 - (1 - Qf)^n) -- the Horvitz-Thompson weight of a member of shared_candidates(n) (0 at row 0 and the EOS row)."""
        n = int(n)
        if n not in self._inclusion:
            _, Qf = self._q()
            V = self.V
            b = np.zeros(V + 2, dtype=np.float64)
            with np.errstate(divide="ignore"):
                b[1:V + 1] = -np.log(-np.expm1(n * np.log1p(-Qf[1:V + 1])))
            self._inclusion[n] = torch.as_tensor(b.astype(np.float32)).to(self.device)
        return self._inclusion[n]

    def batch(self, users, L_enc, L_dec, eos, n_neg, seed, shared_negs=0, hard_negs=0, hard_k=None, hard_skip=0, logq=False):
        if shared_negs > 0 and hard_negs > 0:
            raise ValueError("hard_negs and shared_negs exclude each other: a shared list has no per-position negatives to harden")
        if logq and hard_negs > 0:
            raise ValueError("logq and hard_negs exclude each other: hard columns are not draws from the sampler's distribution")
        users = users.to(self.device).contiguous()
        seqs = hip.assemble_batch(self.items, self.offsets, users, L_enc, L_dec, eos)
        if shared_negs > 0:
            n_items = self.shared_candidates(shared_negs, seed)
        else:
            n_items = hip.sample_negatives(self.excl, self.excl_off, users, n_neg, self.V, seed, self.alias)
        if hard_negs > 0:
            # the private draw as always, and ONE pool for the batch under a seed of its own (the batch seed carries the rank); the
            # users' exclusion rows are handed on as offsets into self.excl, the values are not copied
            from .models import HardNegatives
            k = n_neg // L_dec
            pool = self.shared_candidates(hard_negs, seed ^ HARD_POOL_SEED)
            n_items = HardNegatives(n_items, pool, k if not hard_k else int(hard_k), hard_skip, excl=self.excl,
                                    excl_lo=self.excl_off[users], excl_hi=self.excl_off[users + 1])
        if logq:
            from .models import LogQNegatives
            if shared_negs > 0:
                n_items = LogQNegatives(n_items, cand_bias=self.inclusion_bias(shared_negs)[n_items])
            else:
                neg_bias, _, shift = self.logq_tables()
                n_items = LogQNegatives(n_items, neg_bias=neg_bias, pos_bias=shift[users] + float(np.log(n_neg // L_dec)))
        return seqs, n_items, self.val[users], self.test[users]

    def shared_candidates(self, n, seed):
        """ONE candidate list for a whole batch (models.SharedLogits): the distinct ids among n draws over 1..V, ascending -- the
        device sampler called for one pseudo-user whose exclusion row is empty (frequency-weighted when the domain has an alias table).
        A position's own target may be in the list; the loss leaves it out of that position's sum."""
        if self._no_excl is None:
            self._no_excl = (torch.zeros(1, device=self.device, dtype=torch.int64), torch.zeros(2, device=self.device, dtype=torch.int64),
                             torch.zeros(1, device=self.device, dtype=torch.int64))
        ex, off, user = self._no_excl
        return torch.unique(hip.sample_negatives(ex, off, user, int(n), self.V, seed, self.alias).view(-1))


class DeviceLoader(object):
    """Iterates a DeviceDomain like the reference's DataLoader over pickle_loader (train: num_n * enc_maxlen
    negatives per user; eval_n: candidate_size).  rank / world shard the users as rank::world.
    shared_negs > 0: n_items is ONE 1-D ascending list of the distinct ids among shared_negs draws, shared by the batch, instead of
    the [B, n_neg] per-user draws (every rank draws its own: the batch seed carries the rank).
    hard_negs > 0: n_items is a models.HardNegatives -- the per-user draws plus one pool of the distinct ids among hard_negs draws,
    from which the model's current top scorers replace the first hard_k (None: all) negatives of every position.
    logq=True: n_items is a models.LogQNegatives -- the same draws (or the same shared list) together with the logQ correction of the
    distribution they came from, k = n_neg // L_dec negatives per position."""

    def __init__(self, domain, batch_size, L_enc, L_dec, eos, n_neg, seed=0, shuffle=True, rank=0, world=1, drop_last=True,
                 shared_negs=0, hard_negs=0, hard_k=None, hard_skip=0, logq=False):
        self.dom, self.bs, self.Le, self.Ld, self.eos, self.n_neg = domain, batch_size, L_enc, L_dec, eos, n_neg
        self.shared_negs = int(shared_negs)
        self.hard = (int(hard_negs), hard_k, int(hard_skip))
        self.logq = bool(logq)
        if self.shared_negs > 0 and self.hard[0] > 0:
            raise ValueError("hard_negs and shared_negs exclude each other: a shared list has no per-position negatives to harden")
        if self.logq and self.hard[0] > 0:
            raise ValueError("logq and hard_negs exclude each other: hard columns are not draws from the sampler's distribution")
        if self.logq and self.shared_negs <= 0 and n_neg // L_dec < 1:
            raise ValueError("logq: fewer than one negative per position (n_neg=%d, L_dec=%d)" % (n_neg, L_dec))
        self.users = torch.arange(rank, domain.n, world, device=domain.device)[:max(domain.n // world, 1 if world == 1 else 0)]   # equal shards (dist.shard_users)
        self.shuffle, self.seed, self.epoch, self.drop_last = shuffle, int(seed) * 1000003 + rank, 0, drop_last
        self.seed_rank = (int(seed), int(rank))
        batch_seed(seed, rank, 0)                            # the domain of the packing, checked up front
        n = self.users.numel()
        self.nb = n // batch_size if drop_last else (n + batch_size - 1) // batch_size
        if self.nb < 1:
            raise ValueError("DeviceLoader: fewer users (%d) than batch_size (%d)" % (n, batch_size))

    def __len__(self):
        return self.nb

    def __iter__(self):
        order = self.users
        if self.shuffle:
            g = torch.Generator(device="cpu").manual_seed(self.seed + self.epoch)
            order = order[torch.randperm(order.numel(), generator=g).to(order.device)]
        for i in range(self.nb):
            u = order[i * self.bs:(i + 1) * self.bs]
            seed = batch_seed(self.seed_rank[0], self.seed_rank[1], self.epoch * self.nb + i)
            if self.hard[0] > 0:
                yield self.dom.batch(u, self.Le, self.Ld, self.eos, self.n_neg, seed, 0, *self.hard)
            elif self.logq:
                yield self.dom.batch(u, self.Le, self.Ld, self.eos, self.n_neg, seed, self.shared_negs, logq=True)
            elif self.shared_negs > 0:
                yield self.dom.batch(u, self.Le, self.Ld, self.eos, self.n_neg, seed, self.shared_negs)
            else:
                yield self.dom.batch(u, self.Le, self.Ld, self.eos, self.n_neg, seed)
        self.epoch += 1


class DeviceEvalLoader(object):
    """Evaluation batches in the reference's layout (pickle_loader_eval + test_seq_gen, data_loader.py:39-55,58-150):
    ((eval_enc_in, eval_dec_in, val), (test_enc_in, test_dec_in, test), n_items_f, n_items_r) with candidate_size
    frequency-weighted (n_items_f, when the domain has an alias table) and uniform (n_items_r) candidates that exclude
    the user's items.  The validation input is the sequence, the test input the sequence + [val]."""

    def __init__(self, seqs, val, test, V, device, batch_size, L_enc, L_dec, eos, candidate_size, wf=None, seed=0,
                 rank=0, world=1):
        self.eval_dom = DeviceDomain(seqs, val, test, V, device, exclude_val=True, wf=wf)
        self.test_dom = DeviceDomain([list(s) + [int(v)] for s, v in zip(seqs, val)], val, test, V, device,
                                     exclude_val=True)
        self.bs, self.Le, self.Ld, self.eos, self.C, self.seed = batch_size, L_enc, L_dec, eos, candidate_size, int(seed)
        self.users = torch.arange(rank, len(seqs), world, device=device)     # (evaluation has no collective: shards may differ in size)
        # whole batches only, as the reference's DataLoader(drop_last=True) (data_loader.py:477-482): the last
        # users.numel() % batch_size users are NOT scored; fewer users than one batch give one short batch
        self.nb = max(1, self.users.numel() // batch_size)
        self.epoch = 0

    def __len__(self):
        return self.nb

    def _inputs(self, dom, u):
        enc_in, _, _ = hip.assemble_batch(dom.items, dom.offsets, u, self.Le, self.Ld, self.eos)
        dec_in = torch.cat([torch.zeros_like(enc_in[:, :1]), enc_in[:, :-1]], 1)[:, -self.Ld:].contiguous()   # [0] + enc_in[:-1]
        return enc_in, dec_in

    def __iter__(self):
        for i in range(self.nb):
            u = self.users[i * self.bs:(i + 1) * self.bs].contiguous()
            if u.numel() == 0:
                return
            s = (self.seed << 20) + self.epoch * self.nb + i
            ev = self._inputs(self.eval_dom, u) + (self.eval_dom.val[u],)
            te = self._inputs(self.test_dom, u) + (self.eval_dom.test[u],)
            d = self.eval_dom
            n_r = hip.sample_negatives(d.excl, d.excl_off, u, self.C, d.V, 2 * s)
            n_f = hip.sample_negatives(d.excl, d.excl_off, u, self.C, d.V, 2 * s + 1, d.alias) if d.alias is not None else n_r
            yield ev, te, n_f, n_r
        self.epoch += 1
