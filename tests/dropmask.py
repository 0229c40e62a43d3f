"""Host restatement of the dropout-mask contract of the HIP kernels (recguru_amd/csrc/rg_common.hip.h, DropCfg / rg_hash /
rg_keep / make_drop), in numpy uint32 arithmetic.  Written from the contract and the kernel source, not from kernel output, so
that the GPU tests can hold every dropout site to it element by element (tests/test_dropout_masks_gpu.py).

The contract: element `idx` (a 32-bit, wrapping index in an index space of its own for each site) is decided
  * p == 0.5 : by bit (idx & 31) of rg_hash(seed, idx >> 5),
  * otherwise: by the 16-bit half (idx & 1) of rg_hash(seed, idx >> 1), dropped iff that half < thresh = p * 65536;
and a kept element is scaled by inv_keep = 1 / (1 - p).  Past 2^32 an index space wraps, so masks repeat there."""
import numpy as np

U32 = np.uint32
MASK32 = 0xFFFFFFFF


def _u32(x):
    return np.asarray(x, dtype=np.uint64).astype(np.uint32) if np.asarray(x).dtype != np.uint32 else np.asarray(x)


class DropCfg:
    """make_drop(p, seed) (rg_common.hip.h:472): the 64-bit call seed folded to 32 bits (both halves), the 16-bit threshold,
    the f32 scale of a kept element and the one-bit mode flag.  p is a float on the device: it is rounded to f32 first."""

    def __init__(self, p, seed):
        p32 = np.float32(p)
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        lo, hi = seed & MASK32, seed >> 32
        s = ((lo * 0x9E3779B1) & MASK32) ^ ((hi * 0x85EBCA77 + 0x165667B1) & MASK32)
        s ^= s >> 15
        s = (s * 0x2C1B3C6D) & MASK32
        s ^= s >> 12
        self.seed = s
        self.p = float(p32)
        self.thresh = int(float(p32) * 65536.0 + 0.5) if p32 > 0 else 0
        self.inv_keep = float(np.float32(1.0) / (np.float32(1.0) - p32)) if p32 > 0 else 1.0
        self.onebit = bool(p32 == np.float32(0.5))


def make_drop(p, seed):
    return DropCfg(p, seed)


def rg_hash(seed, x):
    """lowbias32-style hash of (seed, x) (rg_common.hip.h rg_hash), elementwise over a uint32 array."""
    with np.errstate(over="ignore"):
        x = _u32(x) ^ U32(int(seed) & MASK32)
        x = x ^ (x >> U32(16))
        x = x * U32(0x21F0AAAD)
        x = x ^ (x >> U32(15))
        x = x * U32(0x735A2D97)
        x = x ^ (x >> U32(15))
    return x


def keep_bool(cfg, idx):
    """True where element idx (uint32 array) is kept under DropCfg cfg (rg_keep)."""
    idx = _u32(idx)
    if cfg.thresh == 0:
        return np.ones(idx.shape, dtype=bool)
    if cfg.onebit:
        return ((rg_hash(cfg.seed, idx >> U32(5)) >> (idx & U32(31))) & U32(1)).astype(bool)
    h = rg_hash(cfg.seed, idx >> U32(1))
    f = np.where((idx & U32(1)).astype(bool), h >> U32(16), h & U32(0xFFFF))
    return f >= U32(cfg.thresh)


def keep(seed, p, idx):
    """The float64 multiplier of element idx: 0 (dropped) or inv_keep = 1/(1-p) as the kernels hold it (an f32 value)."""
    cfg = make_drop(p, seed)
    return np.where(keep_bool(cfg, idx), cfg.inv_keep, 0.0)


# ---- index spaces: logical coordinates -> the wrapped uint32 index the kernels hash -------------------------------------
def _wrap(x):
    return (np.asarray(x, dtype=np.uint64) & np.uint64(MASK32)).astype(np.uint32)


def lpad(L):
    """rg_lpad: L rounded up to a multiple of 32 (a row of the attention map starts on a hash-word boundary)."""
    return (int(L) + 31) & ~31


def rowmajor_index(row, col, ncols):
    """row * ncols + col for a [rows, ncols] activation, in 32 bits.  The sites that use it:
      dropout_ / dropout_gelu / add_drop_ln / ln_bwd dz_drop   elementwise.hip:1016, 1024 (flat i == m*N + c), 1041, 1074, 410
      gemm_nt EPI_RELU + drop_p (generic kernel, tail)        gemm.hip:189, 223
      gemm_nt EPI_DROP_GELU (weight-stationary kernel)         gemm_ws.hip:261
      embedding gather / scatter (row = token b*L + t)         elementwise.hip:42, 117, 191, 229, 304
      fused FFN block: h1 (ncols = d_ff, seed_h1), out (ncols = d, seed_out)
                                                               fused.hip:596, 641; fused256.hip:283
      ffn_bwd_data's LayerNorm backward (ln=...)              fused.hip:940
      discriminator layer i (row0 + t, ncols = n_i)            disc.hip:94"""
    return _wrap(np.asarray(row, dtype=np.uint64) * np.uint64(ncols) + np.asarray(col, dtype=np.uint64))


def attn_index(b, h, q, key, H, L):
    """((b*H + h)*L + q) * LPAD + key, LPAD = lpad(L), in 32 bits: the attention map (rg_common.hip.h rg_lpad comment).
    Sites: attention.hip:138-155 (fill_dmask, p == 0.5 forward / bf16 backward), 721-727 (forward, 16-bit mode), 902 / 974
    (f32 backward), 1070-1071, 1325, 1451 (bf16 / bf16x3 backward); the single-query kernels use row q = L-1 of the same
    space (attention_lastq.hip:100, 140; attention_lastq_x.hip:294, 426, 671, 763); cross_drop_scale the same space for the
    uniform cross-attention map (elementwise.hip:884-892)."""
    u = np.uint64
    row = (np.asarray(b, dtype=u) * u(H) + np.asarray(h, dtype=u)) * u(L) + np.asarray(q, dtype=u)
    return _wrap(row * u(lpad(L)) + np.asarray(key, dtype=u))


def attn_true_index(b, h, q, key, H, L):
    """The same coordinates as attn_index, unwrapped (Python ints / uint64): where the 32-bit space wraps."""
    return ((int(b) * H + int(h)) * L + int(q)) * lpad(L) + int(key)


# ---- whole masks for the tests -------------------------------------------------------------------------------------------
def rowmajor_mask(seed, p, rows, ncols, row0=0):
    """[rows, ncols] float64 multipliers of a row-major site (rows row0 .. row0 + rows - 1)."""
    r = np.arange(row0, row0 + rows, dtype=np.uint64)[:, None]
    c = np.arange(ncols, dtype=np.uint64)[None, :]
    return keep(seed, p, rowmajor_index(r, c, ncols))


def attn_mask(seed, p, H, L, bs):
    """[len(bs), H, L, L] float64 multipliers of the attention map of the sequences bs (query, key)."""
    bs = np.asarray(list(bs), dtype=np.uint64)
    b = bs[:, None, None, None]
    h = np.arange(H, dtype=np.uint64)[None, :, None, None]
    q = np.arange(L, dtype=np.uint64)[None, None, :, None]
    k = np.arange(L, dtype=np.uint64)[None, None, None, :]
    return keep(seed, p, attn_index(b, h, q, k, H, L))
