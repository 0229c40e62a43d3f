"""float64 restatement of the sampled softmax over ONE candidate list shared by every position (csrc/shared_ce.hip):

    z_pos  = h_t . E[y_t] (+ pos_bias[t]),   z_c = h_t . E[S_c] (+ cand_bias[c]) for every c with S_c != y_t
    loss_t = log(exp(z_pos) + sum_{c: S_c != y_t} exp(z_c)) - z_pos,   loss = sum_t m_t loss_t / count

chunked over the live rows so that no [n, C] matrix of the whole batch is held.  Runs on whatever device its inputs live on."""
import torch


def shared_ce_ref(h, table, labels, cand, mask, skip_row=-1, cand_bias=None, pos_bias=None, count=None, chunk=1024):
    """-> (loss, dh [n, d], dE [rows, d], lse [n]) in float64; count: the normaliser (default sum(mask)); skip_row: the target route
    adds nothing to that row of dE."""
    h64, E = h.detach().double(), table.detach().double()
    n, d = h64.shape
    labels, cand = labels.reshape(-1), cand.reshape(-1)
    m = mask.reshape(-1).double()
    cnt = float(m.sum()) if count is None else float(count)
    live = torch.nonzero(m).reshape(-1)
    Ec = E[cand]
    cb = torch.zeros(cand.numel(), dtype=torch.float64, device=h.device) if cand_bias is None else cand_bias.double()
    pb = torch.zeros(n, dtype=torch.float64, device=h.device) if pos_bias is None else pos_bias.double()
    tot = 0.0
    dh, dE, lse_all = torch.zeros_like(h64), torch.zeros_like(E), torch.zeros(n, dtype=torch.float64, device=h.device)
    for s in range(0, live.numel(), chunk):
        ix = live[s:s + chunk]
        y = labels[ix]
        hx = h64[ix]
        zp = (hx * E[y]).sum(1) + pb[ix]
        zc = hx @ Ec.T + cb[None, :]
        zc = zc.masked_fill(cand[None, :] == y[:, None], float("-inf"))
        z = torch.cat([zp[:, None], zc], 1)
        lse = torch.logsumexp(z, 1)
        lse_all[ix] = lse
        tot += float((m[ix] * (lse - zp)).sum())
        p = torch.exp(z - lse[:, None])
        p[:, 0] -= 1.0
        p *= (m[ix] / cnt)[:, None]
        dh[ix] = p[:, 1:] @ Ec + p[:, :1] * E[y]
        dE.index_add_(0, cand, p[:, 1:].T @ hx)
        keep = y != skip_row
        dE.index_add_(0, y[keep], p[keep, :1] * hx[keep])
    return tot / cnt, dh, dE, lse_all
