"""Drop-in model classes of the hot path, HIP-backed.

Same class names, constructor signatures, method names and state_dict keys as the reference:
  MyAuto4Rec_c   GURU/AutoEnc4Rec_cross.py:17-221   (cross-domain generator)
  MyAuto4Rec     GURU/AutoEnc4Rec.py:136-230        (single-domain autoencoder)
  MyRec          GURU/AutoEnc4Rec.py:20-133         (wrapper: recon + recommender decoder)
  Discriminator  GURU/tools/utils.py:30-57
so reference checkpoints load with load_state_dict and the reference's drivers can call them.
Differences a caller can observe: attention maps are returned only on request
(return_attn=True; every hot-path caller discards them); forward() returns a SampledLogits handle instead of a dense [B,L,k+1]
tensor so that loss_ae can run the fused gather-dot-loss kernel -- call .dense() for the tensor.
"""
import numpy as np
import torch
import torch.nn as nn

from . import blocks, ops


def _f32_mask(ids, pad):
    """(1 - (ids == pad)).float() -- gan_training.py:347-350 and the inline copies."""
    if ids.is_cuda and ids.dtype == torch.int64:
        from . import hip
        return hip.pad_mask(ids.contiguous(), pad)
    return (ids != pad).to(torch.float32)


class SampledLogits(object):
    """Deferred logits of the positive + k sampled negatives per position
    (AutoEnc4Rec_cross.py:201-215).  Holds the decoder states and the item ids.  neg may be a HardNegatives: it becomes the [n, k] ids
    when a loss is asked for, under that loss's mask (resolve_negatives: the positions the loss counts are the ones that are scored).
    neg_bias [table rows] / pos_bias [one per position]: the logQ correction (LogQNegatives), added to the negatives'
    logits by item id and to the positive's logit in the sampled softmax."""

    def __init__(self, h, table, pos, neg, k, skip_row=-1, neg_bias=None, pos_bias=None):
        self.h, self.table, self.pos, self.neg, self.k, self.skip_row = h, table, pos, neg, k, skip_row
        if pos_bias is not None and pos_bias.numel() != pos.numel():
            raise ValueError("pos_bias holds %d values for %d positions" % (pos_bias.numel(), pos.numel()))
        self.neg_bias, self.pos_bias = neg_bias, pos_bias

    def negatives(self, mask=None):
        """The [n, k] negative ids the losses see (mask None: every position counts, what dense() shows)."""
        if isinstance(self.neg, HardNegatives) and mask is None:
            mask = torch.ones(self.pos.numel(), device=self.h.device, dtype=torch.float32)
        return resolve_negatives(self.h, self.table, self.pos, self.neg, self.k, mask)

    def loss(self, mask):
        """SampledCrossEntropyLoss with label 0 and masked mean (tools/lossfunctions.py:36-49)."""
        return ops.sampled_softmax_loss(self.h, self.table, self.pos, self.negatives(mask), mask, self.k, self.skip_row,
                                        neg_bias=self.neg_bias, pos_bias=self.pos_bias)

    def dense(self):
        """The [B, L, 1 + k] logits tensor the reference's forward returns (AutoEnc4Rec_cross.py:211-215: column 0 the
        positive, then the k sampled negatives), f32, forward only (no autograd graph) -- for callers that inspect
        logits; the training losses go through loss() / bpr(), which never materialise it."""
        from . import hip
        d = self.h.shape[-1]
        h2 = self.h.detach().contiguous().view(-1, d)
        neg = self.negatives().contiguous().view(-1, self.k)
        scores, _ = hip.rank_scores(h2, ops.shadow(self.table), self.pos.contiguous().view(-1), neg, want_rank=False)
        if self.pos_bias is not None:                      # the logits the corrected loss sees
            scores[:, 0] += self.pos_bias.reshape(-1).to(torch.float32)
        if self.neg_bias is not None:
            scores[:, 1:] += self.neg_bias.to(torch.float32)[neg]
        return scores.view(tuple(self.h.shape[:-1]) + (self.k + 1,))

    def bpr(self, mask, sas=False):
        """BPRLoss (tools/lossfunctions.py:56-72); sas=True: BPRLoss_sas (:79-96), what train_auto.py uses (:26)."""
        if self.neg_bias is not None or self.pos_bias is not None:
            raise ValueError("BPR is no estimate of a softmax: the logQ correction (neg_bias / pos_bias) serves the sampled softmax only")
        return ops.bpr_loss(self.h, self.table, self.pos, self.negatives(mask), mask, self.k, self.skip_row, sas=sas)


class SharedLogits(object):
    """Deferred logits of the positive + ONE candidate list shared by every position of the batch (cand: 1-D, strictly ascending table
    rows).  A candidate equal to a position's own target is left out of that position's softmax."""

    def __init__(self, h, table, labels, cand, skip_row=-1, cand_bias=None):
        self.h, self.table, self.labels, self.cand, self.skip_row = h, table, labels, cand, skip_row
        self.cand_bias = cand_bias          # [C] f32 or None: the logQ correction of the list (LogQNegatives)

    def loss(self, mask):
        """Sampled softmax with label 0 and masked mean over [z_pos, z_cand minus accidental hits] -- the fused kernels of
        csrc/shared_ce.hip, no logits stored."""
        return ops.shared_softmax_loss(self.h, self.table, self.labels, self.cand, mask, self.skip_row, cand_bias=self.cand_bias)

    def dense(self):
        """The [..., 1 + C] f32 logits (column 0 the positive, then the candidates in list order; accidental hits shown as -inf),
        forward only (no autograd graph) -- for inspection at small shapes; loss() never materialises it."""
        from . import hip
        d = self.h.shape[-1]
        h2 = self.h.detach().contiguous().view(-1, d)
        labels = self.labels.contiguous().view(-1)
        cand = self.cand.contiguous()
        n, C = h2.shape[0], cand.numel()
        out, _ = hip.rank_scores(h2, ops.shadow(self.table), labels, cand.view(1, C).expand(n, C).contiguous(), want_rank=False)
        if self.cand_bias is not None:
            out[:, 1:] += self.cand_bias.to(torch.float32).view(1, C)
        out[:, 1:].masked_fill_(cand.view(1, C) == labels.view(n, 1), float("-inf"))
        return out.view(tuple(self.h.shape[:-1]) + (cand.numel() + 1,))

    def bpr(self, mask, sas=False):
        raise NotImplementedError("BPR takes per-position negatives (a 2-D n_items): a shared candidate list serves the sampled "
                                  "softmax loss only")


class HardNegatives(object):
    """A value for the n_items argument: per-position negatives whose first k_hard columns are the positions' HARD negatives -- ranks
    skip .. skip + k_hard - 1 of one sampled pool under the current model (hip.hard_negs) -- and whose other columns, and
    every slot the pool has no id for, are the ordinary private draw.  private: [B, L * k] (what the loaders yield); pool: 1-D, strictly
    ascending table rows; excl / excl_lo / excl_hi: each sequence's sorted exclusion row excl[excl_lo[b] : excl_hi[b]], or None."""

    def __init__(self, private, pool, k_hard, skip=0, excl=None, excl_lo=None, excl_hi=None):
        if not torch.is_tensor(private) or private.dtype != torch.int64 or private.dim() != 2:
            raise ValueError("HardNegatives: private must be the [B, L * k] int64 draw")
        if not torch.is_tensor(pool) or pool.dtype != torch.int64 or pool.dim() != 1 or pool.numel() < 1:
            raise ValueError("HardNegatives: pool must be a non-empty 1-D int64 list of table rows")
        if int(k_hard) < 1:
            raise ValueError("HardNegatives: k_hard must be at least 1 (got %d)" % int(k_hard))
        if int(skip) < 0:
            raise ValueError("HardNegatives: skip must not be negative (got %d)" % int(skip))
        if (excl_lo is None) != (excl_hi is None) or (excl is None) != (excl_lo is None):
            raise ValueError("HardNegatives: excl, excl_lo and excl_hi come together")
        if excl_lo is not None and (excl_lo.numel() != private.shape[0] or excl_hi.numel() != private.shape[0]):
            raise ValueError("HardNegatives: excl_lo / excl_hi need one entry per sequence (%d)" % private.shape[0])
        self.private, self.pool, self.k_hard, self.skip = private, pool, int(k_hard), int(skip)
        self.excl, self.excl_lo, self.excl_hi = excl, excl_lo, excl_hi

    def to(self, device):
        """The loaders' `n_items.to(device)` (get_next_batch): every tensor moved, the exclusion values shared when already there."""
        mv = lambda t: None if t is None else t.to(device)
        return HardNegatives(mv(self.private), mv(self.pool), self.k_hard, self.skip, mv(self.excl), mv(self.excl_lo), mv(self.excl_hi))


class LogQNegatives(object):
    """A value for the n_items argument: sampled negatives together with the logQ correction of the distribution they were drawn
    from.  ids 2-D [B, L * k] (per-position draws): neg_bias [table rows] = -log Q per item, pos_bias [B] =
    log k - log(1 - m_u) per sequence, either may be None.  ids 1-D (one shared candidate list): cand_bias [C] = -log of each
    candidate's inclusion probability.  The biases are f32 constants: no gradient reaches them."""

    def __init__(self, ids, neg_bias=None, pos_bias=None, cand_bias=None):
        if not torch.is_tensor(ids) or ids.dtype != torch.int64 or ids.dim() not in (1, 2):
            raise ValueError("LogQNegatives: ids must be the [B, L * k] int64 draw or a 1-D int64 candidate list")
        if ids.dim() == 1 and (neg_bias is not None or pos_bias is not None):
            raise ValueError("LogQNegatives: a 1-D candidate list takes cand_bias, not neg_bias / pos_bias")
        if ids.dim() == 2 and cand_bias is not None:
            raise ValueError("LogQNegatives: per-position draws take neg_bias / pos_bias, not cand_bias")
        if cand_bias is not None and cand_bias.numel() != ids.numel():
            raise ValueError("LogQNegatives: cand_bias needs one value per candidate (%d, got %d)" % (ids.numel(), cand_bias.numel()))
        if pos_bias is not None and pos_bias.numel() != ids.shape[0]:
            raise ValueError("LogQNegatives: pos_bias needs one value per sequence (%d, got %d)" % (ids.shape[0], pos_bias.numel()))
        for name, b in (("neg_bias", neg_bias), ("pos_bias", pos_bias), ("cand_bias", cand_bias)):
            if b is not None and (not torch.is_tensor(b) or b.dtype != torch.float32):
                raise ValueError("LogQNegatives: %s must be an f32 tensor" % name)
        self.ids, self.neg_bias, self.pos_bias, self.cand_bias = ids, neg_bias, pos_bias, cand_bias

    def dim(self):
        return self.ids.dim()

    def to(self, device):
        """The loaders' `n_items.to(device)` (get_next_batch): every tensor moved, shared when already there."""
        mv = lambda t: None if t is None else t.to(device)
        return LogQNegatives(mv(self.ids), mv(self.neg_bias), mv(self.pos_bias), mv(self.cand_bias))


def sampled_handle(h, table, labels, n_items, k, skip_row=-1):
    """The deferred-logits handle of a sampled reconstruction loss for any value n_items may take: a 1-D tensor (one shared candidate
    list), a 2-D tensor or a HardNegatives (per-position negatives), or a LogQNegatives around either tensor form."""
    if isinstance(n_items, LogQNegatives):
        if n_items.ids.dim() == 1:
            return SharedLogits(h, table, labels, n_items.ids, skip_row, cand_bias=n_items.cand_bias)
        pb = n_items.pos_bias
        if pb is not None:                                        # one value per sequence -> one per position of labels [B, L]
            B = n_items.ids.shape[0]
            if labels.numel() % B != 0:
                raise ValueError("LogQNegatives: %d sequences of draws for %d labels" % (B, labels.numel()))
            pb = pb.reshape(-1).repeat_interleave(labels.numel() // B)
        return SampledLogits(h, table, labels, n_items.ids, k, skip_row, neg_bias=n_items.neg_bias, pos_bias=pb)
    if torch.is_tensor(n_items) and n_items.dim() == 1:           # one candidate list shared by the batch
        return SharedLogits(h, table, labels, n_items, skip_row)
    return SampledLogits(h, table, labels, n_items, k, skip_row)


def resolve_negatives(h, table, labels, n_items, k, mask):
    """n_items as the item-loss kernels take it.  A plain tensor passes through untouched.  A HardNegatives becomes a fresh [n, k]
    buffer: the private draw, its first k_hard columns overwritten by each live position's hard negatives of the pool, scored with
    the detached decoder states h against the operand-tier copy of table -- no gradient flows through the selection."""
    if isinstance(n_items, LogQNegatives):
        raise ValueError("LogQNegatives serve the sampled reconstruction softmax only (forward(..., recon=True) / the cross model's "
                         "forward): BPR is no estimate of a softmax")
    if not isinstance(n_items, HardNegatives):
        return n_items
    from . import hip
    hn, k = n_items, int(k)
    if not 1 <= hn.k_hard <= k:
        raise ValueError("HardNegatives: need 1 <= k_hard <= k (k_hard=%d, k=%d)" % (hn.k_hard, k))
    d = h.shape[-1]
    h2 = h.detach().contiguous().view(-1, d)
    n = h2.shape[0]
    B = hn.private.shape[0]
    if hn.private.numel() != n * k or n % B != 0:
        raise ValueError("HardNegatives: private holds %d ids, %d positions x k=%d need %d" % (hn.private.numel(), n, k, n * k))
    neg = hn.private.reshape(n, k).clone()
    hip.hard_negs(h2, ops.shadow(table), hn.pool, labels.contiguous().view(-1), mask.reshape(-1).contiguous(), n // B, hn.k_hard,
                  skip=hn.skip, excl=hn.excl, excl_lo=hn.excl_lo, excl_hi=hn.excl_hi, out=neg, checked=True)
    return neg


class FullLogits(object):
    """Deferred logits over the whole catalogue (decoder_neg=False, the reference's `else:` branch): h @ weight.T with weight the
    item table (AutoEnc4Rec.py:228-230: [B, L, V+1]) or projection_{a|b}.weight (AutoEnc4Rec_cross.py:216-220: [B, L, V_{a|b}]).
    Holds the decoder states and the labels (dec_outputs)."""

    def __init__(self, h, weight, labels):
        self.h, self.weight, self.labels = h, weight, labels

    def loss(self, mask):
        """SampledCrossEntropyLoss over all classes with the 1-D label dec_outputs and masked mean (train_auto.py:44-51,
        tools/utils.py:77-84 with neg_sample=False; quirk Q15) -- the fused kernels of csrc/full_ce.hip, no logits stored."""
        return ops.full_softmax_loss(self.h, self.weight, self.labels, mask)

    def dense(self):
        """The [B, L, C] f32 logits tensor the reference's forward returns, forward only (no autograd graph): one HIP GEMM
        (C x B x L x 4 bytes -- for inspection at small shapes; loss() never materialises it)."""
        from . import hip
        d = self.h.shape[-1]
        h2 = self.h.detach().contiguous().view(-1, d)
        out = hip.gemm_nt(h2, ops.shadow(self.weight), out_f32=True)
        return out.view(tuple(self.h.shape[:-1]) + (self.weight.shape[0],))


def check_recon_handle(logits, neg_sample):
    """loss_ae's guard (training.py, auto_training.py): neg_sample must match the handle the model returned -- the reference dies
    on a view over mismatched logits."""
    if not neg_sample and not isinstance(logits, FullLogits):
        raise ValueError("loss_ae(neg_sample=False) needs full-vocabulary logits, but the model returned sampled ones "
                         "(param.decoder_neg=True and n_negs < vocab_size): set param.decoder_neg=False")
    if neg_sample and isinstance(logits, FullLogits):
        raise ValueError("loss_ae(neg_sample=True) needs sampled logits, but the model returned full-vocabulary ones "
                         "(param.decoder_neg=False or n_negs >= vocab_size)")
    return logits


class Discriminator(nn.Module):
    """tools/utils.py:30-57: Linear-ReLU-Drop(.2) x3 + Linear; keys main.0/3/6/9.{weight,bias}."""

    def __init__(self, in_dim, out_dim, mid_dim):
        super(Discriminator, self).__init__()
        if out_dim != 1:
            raise ValueError("Discriminator: out_dim must be 1 (train_gan.py:131)")
        self.main = nn.Sequential(
            nn.Linear(in_dim, mid_dim), nn.ReLU(True), nn.Dropout(p=0.2),
            nn.Linear(mid_dim, mid_dim * 2), nn.ReLU(True), nn.Dropout(p=0.2),
            nn.Linear(mid_dim * 2, mid_dim), nn.ReLU(True), nn.Dropout(p=0.2),
            nn.Linear(mid_dim, out_dim))

    def params(self):
        m = self.main
        return (m[0].weight, m[0].bias, m[3].weight, m[3].bias, m[6].weight, m[6].bias, m[9].weight, m[9].bias)

    def drop_p(self):
        return 0.2 if self.training else 0.0        # nn.Dropout(p=0.2), tools/utils.py:44,47,50

    def forward(self, inputs):
        return ops.DiscriminatorFn.run(inputs, self.drop_p(), *self.params())


class MyAuto4Rec_c(nn.Module):
    def __init__(self, device, param, wf=None, dec_share=False, dec_rec=False, enc_share=True, pos_train=False):
        """pos_train=True: pos_emb_a / pos_emb_b are learned tables (blocks.PositionalEncodingM, max_len = param.enc_maxlen; state keys
        pos_emb_{a|b}.pos_emb.weight, no 'pe' buffers).  The reference's cross model has no such option (AutoEnc4Rec_cross.py:17): it is
        this project's extension, off by default."""
        super(MyAuto4Rec_c, self).__init__()
        self.param = param
        self.device = device
        self.dec_share = dec_share
        self.dec_rec = dec_rec
        self.enc_share = enc_share
        if wf is not None:
            wf = np.power(wf, 0.75)
            self.weights = torch.as_tensor(wf / wf.sum(), dtype=torch.float32)
        else:
            self.weights = None

        def stack(cls):
            return cls(d_model=param.d_model, d_ff=param.d_ff, d_k=param.d_k, d_v=param.d_v,
                       n_heads=param.num_heads, n_layers=param.num_blocks, pad_index=param.pad_index,
                       device=device, dropout=param.dropout_rate)
        # construction order follows the reference so that default initialisation under a given
        # torch seed produces the same state_dict
        def positions():
            if pos_train:
                return blocks.PositionalEncodingM(param.d_model, param.dropout_rate, max_len=param.enc_maxlen, device=device)
            return blocks.PositionalEncoding(param.d_model, param.dropout_rate)
        self.src_emb_a = nn.Embedding(param.vocab_size_a + 1, param.d_model)
        self.pos_emb_a = positions()
        self.src_emb_b = nn.Embedding(param.vocab_size_b + 1, param.d_model)
        self.pos_emb_b = positions()
        if enc_share:
            self.encoder = stack(blocks.EncoderM)
        else:
            self.encoder_a = stack(blocks.EncoderM)
            self.encoder_b = stack(blocks.EncoderM)
        if dec_share:
            self.decoder = stack(blocks.DecoderM)
        else:
            self.decoder_a = stack(blocks.DecoderM)
            self.decoder_b = stack(blocks.DecoderM)
        if not param.decoder_neg:
            # full-catalogue output layer (AutoEnc4Rec_cross.py:76-78), between the decoders and the recommenders as there
            self.projection_a = nn.Linear(param.d_model, param.vocab_size_a, bias=False)
            self.projection_b = nn.Linear(param.d_model, param.vocab_size_b, bias=False)
        if not dec_rec:
            self.recommend_a = stack(blocks.DecoderM)
            self.recommend_b = stack(blocks.DecoderM)

    # ---- helpers ------------------------------------------------------------------------------
    def _emb(self, domain):
        return (self.src_emb_a, self.pos_emb_a) if domain == "a" else (self.src_emb_b, self.pos_emb_b)

    def _embed(self, ids, domain, mask):
        emb, pos = self._emb(domain)
        blocks.check_positions(pos, ids.shape[1])
        return ops.embed_pe(emb.weight, pos.table(), ids, mask, drop_p=pos.drop_p())

    def _encoder(self, domain):
        if self.enc_share:
            return self.encoder
        return self.encoder_a if domain == "a" else self.encoder_b

    # ---- reference surface --------------------------------------------------------------------
    def get_seq_embed(self, enc_inputs, domain="a", mask=None, last_only=False, return_attn=False):
        """AutoEnc4Rec_cross.py:93-115.  The key-pad value is the EOS id vocab_size_{a|b} (quirk Q2).
        last_only=True returns just [:, -1, :] (what every hot-path caller slices out).
        return_attn=True returns (enc_outputs, enc_self_attns [B, n_layers, H, L, L] f32), the reference's tuple (:115)."""
        if return_attn:
            blocks.check_return_attn(self)
        L = enc_inputs.shape[1]
        mask = mask.reshape(-1, L)
        x = self._embed(enc_inputs, domain, mask)
        pad_value = self.param.vocab_size_a if domain == "a" else self.param.vocab_size_b
        return self._encoder(domain)(x, enc_inputs, pad_value, mask, last_only=last_only, return_attn=return_attn)

    def _decode(self, stack, enc_inputs, dec_inputs, domain, mask, d_mask, detach_enc=False, return_attn=False):
        if return_attn:
            blocks.check_return_attn(self)
        L = self.param.enc_maxlen
        u = self.get_seq_embed(enc_inputs, domain, mask.reshape(-1, L), last_only=True)
        if detach_enc:
            u = u.detach()
        x = self._embed(dec_inputs, domain, d_mask)
        return stack(x, u.contiguous(), dec_inputs, enc_inputs, d_mask, return_attn=return_attn)

    def get_dec_out(self, enc_inputs, dec_inputs, domain="a", mask=None, return_attn=False):
        """AutoEnc4Rec_cross.py:117-147: decoder pad mask comes from enc_inputs (quirk Q5).
        return_attn=True fills the two map slots: (dec_outputs, dec_self_attns, dec_enc_attns), each map [B, n_layers, H, L, L] f32."""
        if return_attn:
            blocks.check_return_attn(self)
        d_mask = _f32_mask(enc_inputs, self.param.pad_index)
        if self.dec_share:
            stack = self.decoder
        else:
            stack = self.decoder_a if domain == "a" else self.decoder_b
        if return_attn:
            return self._decode(stack, enc_inputs, dec_inputs, domain, mask, d_mask, return_attn=True)
        return self._decode(stack, enc_inputs, dec_inputs, domain, mask, d_mask), None, None

    def recommend_forward(self, enc_in, dec_in, domain, mask, return_attn=False):
        """AutoEnc4Rec_cross.py:149-183: pad mask from dec_in; encoder state detached if fixed_enc.
        return_attn=True returns (h, dec_self_attns, dec_enc_attns) of the recommender stack."""
        if return_attn:
            blocks.check_return_attn(self)
        d_mask = _f32_mask(dec_in, self.param.pad_index)
        if self.dec_rec:
            stack = self.decoder_a if domain == "a" else self.decoder_b
        else:
            stack = self.recommend_a if domain == "a" else self.recommend_b
        return self._decode(stack, enc_in, dec_in, domain, mask, d_mask, detach_enc=bool(self.param.fixed_enc), return_attn=return_attn)

    def item_table(self, domain):
        return self.src_emb_a.weight if domain == "a" else self.src_emb_b.weight

    def forward(self, enc_inputs, dec_inputs, dec_outputs, n_items, domain, mask):
        """AutoEnc4Rec_cross.py:185-221 -> SampledLogits handle (decoder_neg branch; SharedLogits when n_items is 1-D) or FullLogits over projection_{a|b}
        (the `else:` branch: V_{a|b} classes)."""
        dec_out, _, _ = self.get_dec_out(enc_inputs, dec_inputs, domain, mask)
        vocab = self.param.vocab_size_a if domain == "a" else self.param.vocab_size_b
        if not (self.param.decoder_neg and self.param.n_negs < vocab):
            proj = getattr(self, "projection_a" if domain == "a" else "projection_b", None)
            if proj is None:
                raise ValueError("full-vocabulary logits need projection_%s: construct MyAuto4Rec_c with param.decoder_neg=False "
                                 "(n_negs=%d >= vocab_size_%s=%d)" % (domain, self.param.n_negs, domain, vocab))
            return FullLogits(dec_out, proj.weight, dec_outputs)
        return sampled_handle(dec_out, self.item_table(domain), dec_outputs, n_items, self.param.n_negs)


class MyAuto4Rec(nn.Module):
    def __init__(self, vocab_size, d_model, pad_index, d_ff, d_k, d_v, n_heads, n_layers, device, param,
                 wf=None, pos_train=False):
        super(MyAuto4Rec, self).__init__()
        self.pad_index = pad_index
        self.param = param
        self.device = device
        if wf is not None:
            wf = np.power(wf, 0.75)
            self.weights = torch.as_tensor(wf / wf.sum(), dtype=torch.float32)
        else:
            self.weights = None
        self.src_emb = nn.Embedding(vocab_size + 1, d_model, padding_idx=pad_index)
        if pos_train:       # learned positions (AutoEnc4Rec.py:155-157), in the reference's construction position
            self.pos_emb = blocks.PositionalEncodingM(d_model, param.dropout_rate, max_len=param.enc_maxlen, device=device)
        else:
            self.pos_emb = blocks.PositionalEncoding(d_model, param.dropout_rate)
        self.encoder = blocks.EncoderM(d_model=d_model, d_ff=d_ff, d_k=d_k, d_v=d_v, n_heads=n_heads,
                                       n_layers=n_layers, pad_index=pad_index, device=device,
                                       dropout=param.dropout_rate)
        self.decoder = blocks.DecoderM(d_model=d_model, d_ff=d_ff, d_k=d_k, d_v=d_v, n_heads=n_heads,
                                       n_layers=n_layers, pad_index=pad_index, device=device,
                                       dropout=param.dropout_rate)

    def _embed(self, ids, mask):
        blocks.check_positions(self.pos_emb, ids.shape[1])
        # padding_idx row receives no gradient (AutoEnc4Rec.py:153)
        return ops.embed_pe(self.src_emb.weight, self.pos_emb.table(), ids, mask, skip_row=self.pad_index,
                            drop_p=self.pos_emb.drop_p())

    def get_seq_embed(self, enc_inputs, last_only=False, return_attn=False):
        """AutoEnc4Rec.py:175-184: real pad id for both the row mask and the key mask.
        return_attn=True fills the map slot: (enc_outputs, enc_self_attns [B, n_layers, H, L, L] f32), the reference's tuple (:184)."""
        if return_attn:
            blocks.check_return_attn(self)
        mask = _f32_mask(enc_inputs, self.pad_index)
        x = self._embed(enc_inputs, mask)
        if return_attn:
            return self.encoder(x, enc_inputs, self.pad_index, mask, last_only=last_only, return_attn=True)
        return self.encoder(x, enc_inputs, self.pad_index, mask, last_only=last_only), None

    def decode_with(self, stack, enc_inputs, dec_inputs, detach_enc=False, return_attn=False):
        """The decoder `stack` over the encoder's last state; return_attn=True returns (h, dec_self_attns, dec_enc_attns)."""
        if return_attn:
            blocks.check_return_attn(self)
            blocks.check_return_attn(stack)          # (MyRec's recommender stack is no child of this module)
        u, _ = self.get_seq_embed(enc_inputs, last_only=True)
        if detach_enc:
            u = u.detach()
        mask = _f32_mask(dec_inputs, self.pad_index)
        x = self._embed(dec_inputs, mask)
        return stack(x, u.contiguous(), dec_inputs, enc_inputs, mask, return_attn=return_attn)

    def get_dec_out(self, enc_inputs, dec_inputs, return_attn=False):
        """AutoEnc4Rec.py:186-204: decoder pad mask from dec_inputs.
        return_attn=True fills the two map slots: (dec_outputs, dec_self_attns, dec_enc_attns)."""
        if return_attn:
            return self.decode_with(self.decoder, enc_inputs, dec_inputs, return_attn=True)
        return self.decode_with(self.decoder, enc_inputs, dec_inputs), None, None

    def forward(self, enc_inputs, dec_inputs, dec_outputs, n_items):
        """AutoEnc4Rec.py:206-230 -> SampledLogits handle (sampled branch) or FullLogits over all V+1 rows of src_emb
        (the `else:` branch)."""
        h, _, _ = self.get_dec_out(enc_inputs, dec_inputs)
        if not (self.param.decoder_neg and self.param.n_negs < self.param.vocab_size):
            return FullLogits(h, self.src_emb.weight, dec_outputs)
        return sampled_handle(h, self.src_emb.weight, dec_outputs, n_items, self.param.n_negs, self.pad_index)


class MyRec(nn.Module):
    def __init__(self, device_t, param, wf=None, dec_rec=False, fix_enc=False, sas=False, pos_train=False):
        super(MyRec, self).__init__()
        if sas:
            raise NotImplementedError("the SASRec baseline branch (sas=True) is out of scope (SURVEY.md 2, row 2)")
        self.fix_enc = fix_enc
        self.sas = sas
        self.device = device_t
        self.AutoEnc = MyAuto4Rec(vocab_size=param.vocab_size, d_model=param.d_model, pad_index=0, d_ff=param.d_ff,
                                  d_k=param.d_k, d_v=param.d_v, n_heads=param.num_heads, n_layers=param.num_blocks,
                                  device=device_t, param=param, wf=wf, pos_train=pos_train)
        if not dec_rec:
            self.recommend = blocks.DecoderM(d_model=param.d_model, d_ff=param.d_ff, d_k=param.d_k, d_v=param.d_v,
                                             n_heads=param.num_heads, n_layers=param.num_blocks,
                                             pad_index=param.pad_index, device=device_t, dropout=param.dropout_rate)
        self.dec_rec = dec_rec
        self.param = param

    def get_embedding(self, enc_in, dec_in, return_attn=False):
        """AutoEnc4Rec.py:55-85.  return_attn=True returns (h, dec_self_attns, dec_enc_attns) of the recommender stack (the shared
        decoder with dec_rec), each map [B, n_layers, H, L, L] f32."""
        if return_attn:
            blocks.check_return_attn(self)
        if self.dec_rec:
            out = self.AutoEnc.get_dec_out(enc_in, dec_in, return_attn=return_attn)
            return out if return_attn else out[0]
        return self.AutoEnc.decode_with(self.recommend, enc_in, dec_in, detach_enc=bool(self.fix_enc), return_attn=return_attn)

    def forward(self, enc_in, dec_in, dec_out, n_items, recon=False):
        """AutoEnc4Rec.py:98-133.  recon=True: reconstruction logits handle; else the (p, n) logits of
        the recommender as one SampledLogits handle with k = num_train_neg."""
        if recon:
            return self.AutoEnc(enc_in, dec_in, dec_out, n_items)
        h = self.get_embedding(enc_in, dec_in)
        return SampledLogits(h, self.AutoEnc.src_emb.weight, dec_out, n_items, self.param.num_train_neg, 0)
