"""float64 numpy restatement of the attention-map contract (include/recguru_hip.h: rg_attn_probs, rg_attn_cross_probs,
rg_attn_rollout).  tests/test_attn_maps_cpu.py pins it to the reference's own maps (tests/golden/attn_maps_case*.npz)."""
import numpy as np

NEG_FILL = -1e9


def probs(q, k, key_ids, pad_value, causal, scale):
    """q, k [B, H, L, dk]; key_ids [B, L] -> softmax(mask(q k^T * scale)) [B, H, L, L] float64.  masked(q, key) = key_ids[b, key] ==
    pad_value or (causal and key > q); masked scores are REPLACED by -1e9, so a row without a visible key is uniform over all L keys."""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    L = q.shape[2]
    s = np.einsum("bhqd,bhkd->bhqk", q, k) * np.float64(scale)
    masked = np.broadcast_to((np.asarray(key_ids) == pad_value)[:, None, None, :], s.shape).copy()
    if causal:
        masked |= np.triu(np.ones((L, L), bool), 1)[None, None]
    s = np.where(masked, NEG_FILL, s)
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def split_heads(qkv, H, dk=32):
    """token-major qkv [B, L, 3*H*dk] -> (q, k) each [B, H, L, dk]"""
    B, L, _ = qkv.shape
    P = H * dk
    q = qkv[:, :, :P].reshape(B, L, H, dk).transpose(0, 2, 1, 3)
    k = qkv[:, :, P:2 * P].reshape(B, L, H, dk).transpose(0, 2, 1, 3)
    return q, k


def visible(key_ids, pad_value, causal):
    """[B, L, L] bool: key is visible to query (the complement of the mask)"""
    key_ids = np.asarray(key_ids)
    B, L = key_ids.shape
    vis = np.broadcast_to((key_ids != pad_value)[:, None, :], (B, L, L)).copy()
    if causal:
        vis &= ~np.triu(np.ones((L, L), bool), 1)[None]
    return vis


def cross_probs(enc_ids, pad_value, L, H):
    """The decoder-encoder map over L copies of one encoder state: float32(1) / float32(n_b) at the keys with enc_ids != pad_value,
    0 at the others, float32(1) / float32(L) everywhere if there is none -> [B, H, L, L] float32 (the reference's bits)."""
    enc_ids = np.asarray(enc_ids)
    B = enc_ids.shape[0]
    assert enc_ids.shape[1] == L
    out = np.zeros((B, H, L, L), np.float32)
    for b in range(B):
        live = enc_ids[b] != pad_value
        n = int(live.sum())
        row = np.where(live, np.float32(1) / np.float32(n), np.float32(0)) if n else np.full(L, np.float32(1) / np.float32(L))
        out[b] = row.astype(np.float32)[None, None, :]
    return out


def rollout(maps, query=None, alpha=0.5):
    """maps [B, N, H, L, L]; query [B] or None = L - 1 -> [B, L] float64: r = e_query; for l = N-1 .. 0:
    r <- alpha r + (1 - alpha) (r . mean_h maps[b, l])."""
    maps = np.asarray(maps, np.float64)
    B, N, H, L, _ = maps.shape
    out = np.zeros((B, L), np.float64)
    for b in range(B):
        r = np.zeros(L, np.float64)
        r[L - 1 if query is None else int(query[b])] = 1.0
        for l in range(N - 1, -1, -1):
            abar = maps[b, l].sum(0) / H
            r = alpha * r + (1.0 - alpha) * (r @ abar)
        out[b] = r
    return out
