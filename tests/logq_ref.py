"""Float64 numpy restatement of the logQ-corrected sampled softmax, written from the definitions alone: nothing here
is taken from the library.

Per-position form.  Position t with label y_t and negatives neg[t, 0..k-1]:
    z_0 = h_t . E[y_t] + pos_bias[t]                 z_j = h_t . E[neg[t, j-1]] + neg_bias[neg[t, j-1]]     (j = 1..k)
    l_t = logsumexp(z) - z_0                         loss = sum_t m_t l_t / sum_t m_t
    dl_t/dz_j = softmax(z)_j - [j == 0]              dh_t = w_t sum_j dl_t/dz_j E[row_j],  dE[row_j] += w_t dl_t/dz_j h_t,  w_t = m_t / sum m
Shared form.  One list S for every position; a candidate equal to the position's own label leaves its sum:
    l_t = log(exp(z_0) + sum_{c: S_c != y_t} exp(h_t . E[S_c] + cand_bias[c])) - z_0
Host tables of a sampler that draws item i of 1..V with probability Q_i (Q = w / sum w, w = wf^0.75, w[0] = 0; 1/V without wf):
    neg_bias[i] = -log Qf_i  (Qf: Q with its zeros raised to the smallest positive Q), 0 at row 0 and the EOS row V + 1
    m_u         = sum of Q over user u's exclusion row
    inclusion   = -log(1 - (1 - Qf_i)^N), the probability that i is among N draws
"""
import numpy as np


def _f64(x):
    return None if x is None else np.asarray(x, dtype=np.float64)


def logq_loss_ref(h, table, pos, neg, mask, neg_bias=None, pos_bias=None, skip_row=-1):
    """-> loss, lse [n], dh [n, d], dE [rows, d], per-position losses [n] (0 where masked).  h [n, d], table [rows, d], pos [n],
    neg [n, k], mask [n]; masked positions are never looked at (their ids and biases may hold anything)."""
    h, table, mask = _f64(h), _f64(table), _f64(mask).reshape(-1)
    pos, neg = np.asarray(pos, dtype=np.int64).reshape(-1), np.asarray(neg, dtype=np.int64)
    n, d = h.shape
    R = table.shape[0]
    live = np.nonzero(mask)[0]
    nl = len(live)
    neg = neg.reshape(n, -1)
    rows = np.concatenate([pos[live, None], neg[live]], axis=1)                  # [live, 1 + k]: only live positions are looked at
    z = np.take_along_axis(h[live] @ table.T, rows, axis=1)                      # every dot in float64
    if pos_bias is not None:
        z[:, 0] += _f64(pos_bias).reshape(-1)[live]
    if neg_bias is not None:
        z[:, 1:] += _f64(neg_bias)[rows[:, 1:]]
    mx = z.max(1)
    lse_l = mx + np.log(np.exp(z - mx[:, None]).sum(1))
    c = np.exp(z - lse_l[:, None])
    c[:, 0] -= 1.0
    cnt = mask.sum()
    c *= (mask[live] / cnt)[:, None]
    # W[t, r] = sum of position t's coefficients on table row r (a row may be named more than once): dh = W E, dE = W^T h
    W = np.bincount((np.arange(nl)[:, None] * R + rows).reshape(-1), weights=c.reshape(-1), minlength=nl * R).reshape(nl, R)
    lse, per, dh = np.zeros(n), np.zeros(n), np.zeros((n, d))
    lse[live], per[live], dh[live] = lse_l, lse_l - z[:, 0], W @ table
    if skip_row >= 0:
        W[:, skip_row] = 0.0
    dE = W.T @ h[live]
    return (per * mask).sum() / cnt, lse, dh, dE, per


def shared_loss_ref(h, table, labels, cand, mask, cand_bias=None, pos_bias=None):
    """-> loss, per-position losses [n] of the shared form (accidental hits leave the sum)."""
    h, table, mask = _f64(h), _f64(table), _f64(mask).reshape(-1)
    labels, cand = np.asarray(labels, dtype=np.int64).reshape(-1), np.asarray(cand, dtype=np.int64).reshape(-1)
    cb, pb = _f64(cand_bias), _f64(pos_bias)
    n = h.shape[0]
    per = np.zeros(n)
    zc_all = h @ table[cand].T + (0.0 if cb is None else cb[None, :])
    for t in range(n):
        if mask[t] == 0:
            continue
        z0 = table[labels[t]] @ h[t] + (0.0 if pb is None else pb[t])
        z = np.concatenate([[z0], zc_all[t][cand != labels[t]]])
        mx = z.max()
        per[t] = mx + np.log(np.exp(z - mx).sum()) - z0
    return (per * mask).sum() / mask.sum(), per


def full_loss_ref(h, table, labels, mask, rows=None):
    """The softmax over the catalogue (rows: the ids that count, default every row of the table) -> loss, per-position losses."""
    h, table, mask = _f64(h), _f64(table), _f64(mask).reshape(-1)
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    rows = np.arange(table.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
    z = h @ table[rows].T
    mx = z.max(1)
    lse = mx + np.log(np.exp(z - mx[:, None]).sum(1))
    per = (lse - np.einsum("nd,nd->n", h, table[labels])) * (mask != 0)
    return (per * mask).sum() / mask.sum(), per


def q_of(V, wf=None):
    """(Q, Qf) over rows 0 .. V + 1."""
    Q = np.zeros(V + 2, dtype=np.float64)
    if wf is None:
        Q[1:V + 1] = 1.0 / V
    else:
        w = np.power(np.asarray(wf, dtype=np.float64), 0.75)
        w[0] = 0.0
        m = min(len(w), V + 1)
        Q[1:m] = w[1:m]
        Q = Q / Q.sum()
    Qf = Q.copy()
    floor = min(q for q in Q[1:V + 1] if q > 0)
    for i in range(1, V + 1):
        if Qf[i] <= 0:
            Qf[i] = floor
    return Q, Qf


def neg_bias_table(V, wf=None):
    _, Qf = q_of(V, wf)
    out = np.zeros(V + 2)
    out[1:V + 1] = -np.log(Qf[1:V + 1])
    return out


def exclusion_mass(V, excl_rows, wf=None):
    """m_u of every user: excl_rows = one iterable of excluded ids per user."""
    Q, _ = q_of(V, wf)
    return np.array([sum(Q[int(i)] for i in set(int(j) for j in row)) for row in excl_rows], dtype=np.float64)


def pos_bias_of(m_u, k, V, wf=None):
    """log k - log(1 - m_u), with 1 - m_u no smaller than the smallest positive Q."""
    _, Qf = q_of(V, wf)
    return np.log(float(k)) - np.log(np.maximum(1.0 - np.asarray(m_u, dtype=np.float64), Qf[1:V + 1].min()))


def inclusion_bias_table(V, N, wf=None):
    """-log P(i among N draws) = -log(1 - (1 - Qf_i)^N); 0 at row 0 and the EOS row."""
    _, Qf = q_of(V, wf)
    out = np.zeros(V + 2)
    with np.errstate(divide="ignore"):
        out[1:V + 1] = -np.log(-np.expm1(N * np.log1p(-Qf[1:V + 1])))
    return out


def fixture(seed, V=200, n=96, k=512, d=64):
    """The issue's fixture: Zipf frequencies f_i = i^-1.1, Q ~ f^0.75 over 1..V; item rows whose scores correlate with log Q along one
    direction u (popular items score higher, as in a trained model); one random label per position and k negatives drawn from Q
    with the label's mass removed (m_u = Q_y).  Table rows 0..V (row 0 unused, never drawn)."""
    rng = np.random.RandomState(seed)
    f = np.zeros(V + 1)
    f[1:] = np.arange(1, V + 1, dtype=np.float64) ** -1.1
    Q = f ** 0.75
    Q[0] = 0.0
    Q /= Q.sum()
    u = rng.randn(d)
    u /= np.linalg.norm(u)
    lq = np.log(Q[1:])
    E = np.zeros((V + 1, d))
    E[1:] = 0.35 * rng.randn(V, d) + 0.6 * (lq - lq.mean())[:, None] * u[None, :]
    h = 0.35 * rng.randn(n, d) + u[None, :]
    y = rng.randint(1, V + 1, size=n)
    neg = np.zeros((n, k), dtype=np.int64)
    for t in range(n):
        p = Q.copy()
        p[y[t]] = 0.0
        p /= p.sum()
        neg[t] = rng.choice(V + 1, size=k, p=p)
    neg_bias = np.zeros(V + 1)
    neg_bias[1:] = -lq
    pos_bias = np.log(float(k)) - np.log(1.0 - Q[y])
    return dict(h=h, E=E, y=y, neg=neg, Q=Q, neg_bias=neg_bias, pos_bias=pos_bias, mask=np.ones(n), items=np.arange(1, V + 1))


def shared_fixture(seed, V=2000, N=1024, n=96, d=64):
    """As fixture(), with ONE list for all positions: the distinct ids among N draws from Q, and its inclusion-probability biases."""
    fx = fixture(seed, V=V, n=n, k=1, d=d)
    rng = np.random.RandomState(seed + 1000)
    cand = np.unique(rng.choice(V + 1, size=N, p=fx["Q"]))
    fx["cand"] = cand
    fx["cand_bias"] = -np.log(-np.expm1(N * np.log1p(-fx["Q"][cand])))
    return fx
