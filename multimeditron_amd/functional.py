"""torch.autograd.Function wrappers: each forward/backward is one or a few libmmhip calls.  Activations are
2-D token-major tensors [T, features] throughout (T = batch * seq), which is exactly what the GEMMs consume, so the
path contains no transposes or permutes.

Weight gradients are written straight into `param.grad` by the wgrad GEMM (overwrite on the first contribution of a
step, accumulate afterwards) instead of being returned to autograd: no extra pass over 8 B parameters, and the DP
trainer can point `.grad` at its flat all-reduce buckets.  See `grad_target`."""
from __future__ import annotations

import weakref
from typing import Callable, Optional

import torch

from . import kernels as K
from ._lib import EPI_GELU_ERF, EPI_QUICK_GELU, GELU_KIND, get_option, lib  # noqa: F401

# called as hook(param) right after a parameter's gradient for this step is complete (DP bucket scheduling)
_grad_ready_hook: Optional[Callable] = None


def set_grad_ready_hook(fn: Optional[Callable]):
    global _grad_ready_hook
    _grad_ready_hook = fn


def grad_target(p: torch.Tensor):
    """-> (grad buffer, accumulate?) for writing p's gradient in place."""
    if p.grad is None:
        view = getattr(p, "_mm_grad_view", None)
        if view is None and getattr(p, "_mm_flat", None) is not None:
            p._mm_flat.ensure_grad()          # packed model: gradients live in the flat buffer (fused groups need it)
            view = p._mm_grad_view
        p.grad = view if view is not None else torch.empty_like(p)
        fresh = True
    else:
        fresh = bool(getattr(p, "_mm_fresh", False))
    p._mm_fresh = False
    return p.grad, not fresh


def _ready(p):
    if _grad_ready_hook is not None:
        _grad_ready_hook(p)


# ---- deferred weight gradients ---------------------------------------------------------------------------------------
# The modality backward (ViT-L/14 on 4 images: ~700 short, latency-bound launches) runs at the very end of backward with
# nothing beside it.  Weight-gradient GEMMs have no consumer inside backward, so those of the LAST decoder layers to run
# (layers 0..n-1) are held back and launched on a side stream when backward reaches the embedding splice: they fill the
# CUs the modality backward leaves idle.  Same kernels, same operands, same single write per parameter.
_defer = None


def set_wgrad_deferral(stream, params):
    """stream: side HIP stream for the deferred GEMMs; params: the first Parameter of every deferred group (held weakly).
    stream=None disables."""
    global _defer
    _defer = None if stream is None else {"stream": stream, "params": {id(p): weakref.ref(p) for p in params}, "items": [],
                                          "event": None}


def _is_deferred(p):
    r = _defer["params"].get(id(p)) if _defer is not None else None
    return r is not None and r() is p        # the weak reference guards against id() reuse by a later model


def _target(p):
    return p.grad_target() if isinstance(p, ParamGroup) else grad_target(p)


def _announce(p):
    p.ready() if isinstance(p, ParamGroup) else _ready(p)


def _write_grads(kernel, args, p, q=None):
    """THE gradient write, of one Parameter / ParamGroup p or of the two (p, q) that one launch writes (a LayerNorm's weight and bias,
    xIELU's scalars).  Nothing happens unless all of them train; else kernel(*args, buffer(s)..., accumulate flag(s)...) on their
    grad_target, then the ready hooks.  -> whether the launch ran.  The kernel and its leading arguments travel apart so that a call
    site on the ViT's backward (some 700 short launches) builds no closure."""
    if not (p.requires_grad and (q is None or q.requires_grad)):
        return False
    group = isinstance(p, ParamGroup)               # spelled out for p, the common case: two calls fewer per write
    g, acc = p.grad_target() if group else grad_target(p)
    if q is None:
        kernel(*args, g, acc)
    else:
        g2, acc2 = _target(q)
        kernel(*args, g, g2, acc, acc2)
    p.ready() if group else _ready(p)
    if q is not None:
        _announce(q)
    return True


def _wgrad(dy, x, wg):
    """The weight-gradient GEMM of one parameter group: now on this stream, or held back."""
    if wg.requires_grad and _is_deferred(wg.params[0]):
        _defer["items"].append((dy, x, wg))
        return
    _write_grads(K.linear_wgrad, (dy, x), wg)


def _proj_backward(dy, x, wg, bg, need_dx):
    """THE backward of y = x @ W^T + b, in this order: the bias gradient (column sums of dy), the weight gradient (`_wgrad`: skipped
    for a frozen group, held back for a deferred one), then dx if the input needs one."""
    if bg is not None:
        _write_grads(K.colsum, (dy,), bg)
    _wgrad(dy, x, wg)
    return K.linear_dgrad(dy, wg.tensor()) if need_dx else None


def flush_deferred_wgrads():
    """Launch what has been held back (no-op when nothing is pending); returns the event the compute stream must wait for
    before gradients are read (or None)."""
    d = _defer
    if d is None:
        return None
    if d["items"]:
        main, side = torch.cuda.current_stream(), d["stream"]
        side.wait_stream(main)
        persist = get_option("gemm_persist")         # restore what the trainer / the user had set, not a constant
        lib().mm_set_option(b"gemm_persist", 0)      # one tile per workgroup: shares the chip with the other stream's kernels
        try:
            with torch.cuda.stream(side):
                for dy, x, wg in d["items"]:
                    dy.record_stream(side)
                    x.record_stream(side)
                    _write_grads(K.linear_wgrad, (dy, x), wg)
                ev = torch.cuda.Event()
                ev.record(side)
        finally:
            lib().mm_set_option(b"gemm_persist", persist)
        d["items"].clear()
        d["event"] = ev
    ev, d["event"] = d["event"], None
    return ev


class ParamGroup:
    """One or several Parameters that are adjacent views of one flat buffer and act as a single GEMM operand
    (fused q/k/v, fused gate/up).  `.tensor()` is the fused [sum_out, in] weight (or [sum_out] bias)."""

    def __init__(self, params):
        self.params = list(params)

    def _fused(self, get):
        ts = [get(p) for p in self.params]
        if len(ts) == 1:
            return ts[0]
        first = ts[0]
        if any(t is None for t in ts):
            return None
        ptr = first.data_ptr()
        base = first.untyped_storage().data_ptr()
        for t in ts:
            if t.data_ptr() != ptr or not t.is_contiguous() or t.untyped_storage().data_ptr() != base:
                return None
            ptr += t.numel() * t.element_size()
        rows = sum(t.shape[0] for t in ts)
        shape = (rows,) + tuple(first.shape[1:])
        return first.as_strided(shape, first.stride())

    def tensor(self):
        t = self._fused(lambda p: p.data)
        if t is None:  # not packed (e.g. a freshly constructed CPU->GPU model before pack_parameters)
            raise RuntimeError("fused parameter group is not contiguous in memory: call model.pack_parameters()")
        return t

    @property
    def requires_grad(self):
        for p in self.params:           # a loop, not any(...): asked on every launch of a backward that the host bounds
            if p.requires_grad:
                return True
        return False

    def grad_target(self):
        tg = [grad_target(p) for p in self.params]
        if len(tg) == 1:
            return tg[0]
        accs = {a for _, a in tg}
        g = self._fused(lambda p: p.grad)
        if g is None or len(accs) != 1:
            raise RuntimeError("fused parameter group has non-contiguous .grad buffers")
        return g, accs.pop()

    def ready(self):
        if _grad_ready_hook is not None:
            for p in self.params:
                _grad_ready_hook(p)


def as_group(p):
    return p if isinstance(p, ParamGroup) else ParamGroup([p])


# --------------------------------------------------------------------------------------------------- linear
def _gemm_rows(dy):
    """dy as a GEMM operand: unit last stride, row stride a multiple of 8 elements; a copy only if it is not one already"""
    return dy.contiguous() if dy.stride(-1) != 1 or (dy.stride(0) % 8) else dy


def _linear_forward(fwd, act_fwd, x, w, b, residual, act, keep_pre, *ldc_pad):
    """-> (pre, y) of y = act(x @ W^T + b) + residual, for LinearFn (fwd, act_fwd = K.linear_fwd, K.linear_act_fwd) and GroupedLinearFn
    (their _batched forms, w and b lists): the two differ in nothing else.  An activation whose node someone needs a gradient from
    keeps its pre-activation: act_fwd writes it AND y in one launch where the shape qualifies (None otherwise), else the projection +
    bias alone, the GELU and the add are three launches.  Everything else is one GEMM with its epilogue, pre = None."""
    if not keep_pre:
        return None, fwd(x, w, b, residual, act, *ldc_pad)
    both = act_fwd(x, w, b, act, residual)
    if both is not None:
        return both
    pre = fwd(x, w, b)
    y = K.gelu_fwd(pre, GELU_KIND[act])
    return pre, (K.add(y, residual) if residual is not None else y)


class LinearFn(torch.autograd.Function):
    """y = act(x @ W^T + b) + residual.  x, y 2-D.  W/b are ParamGroups (not autograd inputs); `dummy` is a
    requires-grad scalar that keeps the node in the graph when only the weights need gradients."""

    @staticmethod
    def forward(ctx, x, residual, dummy, wg: ParamGroup, bg: Optional[ParamGroup], act: int, ldc_pad: bool):
        w = wg.tensor()
        b = bg.tensor() if bg is not None else None
        pre, y = _linear_forward(K.linear_fwd, K.linear_act_fwd, x, w, b, residual, act, act and (x.requires_grad or wg.requires_grad), ldc_pad)
        ctx.wg, ctx.bg, ctx.act = wg, bg, act
        ctx.has_res = residual is not None
        ctx.save_for_backward(x, pre)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, pre = ctx.saved_tensors
        dy = _gemm_rows(dy)                       # a copy only when the strides ask for one (GroupedLinearFn: always)
        dres = dy if ctx.has_res else None
        if ctx.act:
            dy = K.gelu_bwd(pre, dy, GELU_KIND[ctx.act])
        return _proj_backward(dy, x, ctx.wg, ctx.bg, ctx.needs_input_grad[0]), dres, None, None, None, None, None


def linear(x, wg, bg=None, residual=None, act=0, ldc_pad=False, dummy=None):
    return LinearFn.apply(x, residual, dummy, as_group(wg), as_group(bg) if bg is not None else None, act, ldc_pad)


# --------------------------------------------------------------------------------------------------- norms
def _reduce_into(p, partials):
    """the gradient of a norm weight / bias p from its backward kernel's per-workgroup partial sums"""
    _write_grads(K.reduce_partials, (partials,), p)


class RMSNormFn(torch.autograd.Function):
    """-> (y, x_res): x_res aliases x and is what the caller feeds to the residual add, so the gradient of the residual
    branch arrives HERE and is added inside the norm-backward kernel (no separate autograd accumulation pass)."""

    @staticmethod
    def forward(ctx, x, dummy, w, eps):
        y, rstd = K.rmsnorm_fwd(x, w.data, eps)
        ctx.w = w
        ctx.save_for_backward(x, rstd)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dres):
        x, rstd = ctx.saved_tensors
        w = ctx.w
        if dy is None:
            return dres, None, None, None
        dx, dwp = K.rmsnorm_bwd(dy.contiguous(), x, w.data, rstd, dres.contiguous() if dres is not None else None)
        _reduce_into(w, dwp)
        return dx, None, None, None


def rmsnorm(x, w, eps, dummy=None):
    return RMSNormFn.apply(x, dummy, w, eps)


class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dummy, w, b, eps):
        y, mean, rstd = K.layernorm_fwd(x, w.data, b.data, eps)
        ctx.w, ctx.b = w, b
        ctx.save_for_backward(x, mean, rstd)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dres):
        x, mean, rstd = ctx.saved_tensors
        w, b = ctx.w, ctx.b
        if dy is None:
            return dres, None, None, None, None
        dx, dwp, dbp = K.layernorm_bwd(dy.contiguous(), x, w.data, mean, rstd, dres.contiguous() if dres is not None else None)
        # dw and db in one launch when both train, else one reduction for the one that does
        if not _write_grads(K.reduce_partials2, (dwp, dbp), w, b):
            _reduce_into(w, dwp)
            _reduce_into(b, dbp)
        return dx, None, None, None, None


def layernorm(x, w, b, eps, dummy=None):
    return LayerNormFn.apply(x, dummy, w, b, eps)


# --------------------------------------------------------------------------------------------------- grouped (expert-major)
# The MoE image modality's E expert towers as ONE chain: activations are expert-major [E * R, C] (expert e owns rows
# [e R, (e + 1) R)), every op whose operands differ per expert takes the experts' parameters as lists and runs one grouped
# launch (kernels.*_batched).  Gradients go where LinearFn / LayerNormFn put them: through grad_target, then _ready.
def _grouped_grad_write(slots, batched, single, partly=None):
    """One gradient write for E experts.  slots[k][e]: expert e's k-th parameter of the write (a ParamGroup or a Parameter; a
    LayerNorm's write has two slots, weight and bias).
      * all train, and each slot's experts agree on overwrite / accumulate: batched(bufs..., accs...), one launch;
      * all train, but the experts disagree: single(e, bufs..., accs...) per expert; either way the ready hooks follow, by expert;
      * some are frozen: partly(e) for every expert -- by default `single` and the hooks for an expert whose slots all train."""
    slots = [[as_group(g) for g in s] for s in slots]
    E = len(slots[0])

    def single_if_live(e):
        _write_grads(single, (e,), *[s[e] for s in slots])

    if not all(g.requires_grad for s in slots for g in s):
        for e in range(E):
            (partly or single_if_live)(e)
        return
    tg = [[g.grad_target() for g in s] for s in slots]
    bufs, accs = [[t for t, _ in s] for s in tg], [[a for _, a in s] for s in tg]
    if all(a == s[0] for s in accs for a in s):
        batched(*bufs, *[s[0] for s in accs])
    else:
        for e in range(E):
            single(e, *[b[e] for b in bufs], *[a[e] for a in accs])
    for e in range(E):
        for s in slots:
            s[e].ready()


class GroupedLinearFn(torch.autograd.Function):
    """LinearFn for E experts at once: x [E*R, K] expert-major, wgs / bgs = one ParamGroup per expert."""

    @staticmethod
    def forward(ctx, x, residual, dummy, wgs, bgs, act: int):
        ws = [wg.tensor() for wg in wgs]
        bs = [bg.tensor() for bg in bgs] if bgs is not None else None
        pre, y = _linear_forward(K.linear_fwd_batched, K.linear_act_fwd_batched, x, ws, bs, residual, act,
                                 act and (x.requires_grad or any(wg.requires_grad for wg in wgs)))
        ctx.wgs, ctx.bgs, ctx.act = wgs, bgs, act
        ctx.has_res = residual is not None
        ctx.save_for_backward(x, pre)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, pre = ctx.saved_tensors
        wgs, bgs = ctx.wgs, ctx.bgs
        E = len(wgs)
        dy = dy.contiguous()                      # unconditionally, where LinearFn (_gemm_rows) copies only when the strides require it
        dres = dy if ctx.has_res else None
        if ctx.act:
            dy = K.gelu_bwd(pre, dy, GELU_KIND[ctx.act])
        R = dy.shape[0] // E
        rows = [slice(e * R, (e + 1) * R) for e in range(E)]
        if bgs is not None:
            _grouped_grad_write([bgs], lambda gs, acc: K.colsum_batched(dy, gs, acc), lambda e, g, acc: K.colsum(dy[rows[e]], g, acc))
        _grouped_grad_write([wgs], lambda gs, acc: K.linear_wgrad_batched(dy, x, gs, acc),
                            lambda e, g, acc: K.linear_wgrad(dy[rows[e]], x[rows[e]], g, acc),
                            partly=lambda e: _wgrad(dy[rows[e]], x[rows[e]], wgs[e]))       # _wgrad: skips a frozen group, honours deferral
        dx = K.linear_dgrad_batched(dy, [wg.tensor() for wg in wgs]) if ctx.needs_input_grad[0] else None
        return dx, dres, None, None, None, None


def grouped_linear(x, wgs, bgs=None, residual=None, act=0, dummy=None):
    return GroupedLinearFn.apply(x, residual, dummy, [as_group(w) for w in wgs], [as_group(b) for b in bgs] if bgs is not None else None, act)


class GroupedLayerNormFn(torch.autograd.Function):
    """LayerNormFn for E experts at once: x [E*R, H] expert-major, ws / bs = one weight / bias Parameter per expert."""

    @staticmethod
    def forward(ctx, x, dummy, ws, bs, eps):
        y, mean, rstd = K.layernorm_fwd_batched(x, [w.data for w in ws], [b.data for b in bs], eps)
        ctx.ws, ctx.bs = ws, bs
        ctx.save_for_backward(x, mean, rstd)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dres):
        x, mean, rstd = ctx.saved_tensors
        ws, bs = ctx.ws, ctx.bs
        E = len(ws)
        if dy is None:
            return dres, None, None, None, None
        dx, dwp, dbp = K.layernorm_bwd_batched(dy.contiguous(), x, [w.data for w in ws], mean, rstd,
                                               dres.contiguous() if dres is not None else None)
        nb = dwp.shape[0] // E
        blocks = [slice(e * nb, (e + 1) * nb) for e in range(E)]

        def partly(e):                                   # some norm is partly frozen: one reduction per trainable parameter
            _reduce_into(ws[e], dwp[blocks[e]])
            _reduce_into(bs[e], dbp[blocks[e]])

        _grouped_grad_write([ws, bs], lambda gw, gb, aw, ab: K.reduce_partials2_batched(dwp, dbp, gw, gb, aw, ab),
                            lambda e, gw, gb, aw, ab: K.reduce_partials2(dwp[blocks[e]], dbp[blocks[e]], gw, gb, aw, ab), partly)
        return dx, None, None, None, None


def grouped_layernorm(x, ws, bs, eps, dummy=None):
    return GroupedLayerNormFn.apply(x, dummy, ws, bs, eps)


# --------------------------------------------------------------------------------------------------- attention
def qkv_views(buf, B, S, Hq, Hkv, D, v_of=None):
    """THE q|k|v split: the q, k, v views [B, S, heads, D] of a fused projection output [T, (Hq+2Hkv)*D] (or of its gradient).
    v_of: the fused buffer v is taken from when buf holds q|k alone (Qwen3's normed, roped copy `qk`, and its gradient)."""
    v = buf if v_of is None else v_of
    return (buf[:, : Hq * D].view(B, S, Hq, D), buf[:, Hq * D:(Hq + Hkv) * D].view(B, S, Hkv, D),
            v[:, (Hq + Hkv) * D:].view(B, S, Hkv, D))


def _attn_grad_like(t, atomics=True):
    """the buffer an attention backward writes the gradient of t into: the fp32 flash backward accumulates with atomics and needs zeros"""
    return torch.zeros_like(t) if atomics and t.dtype == torch.float32 else torch.empty_like(t)


def _rope_attention_forward(qkv, cos, sin, key_mask, dims, roped=False, qkn=None):
    """The RoPE stage, then flash attention, on a fused projection output qkv -> (out, lse, qk, rstd).  The stage is one of: nothing
    (cos is None, or `roped`: the projection's epilogue did it), RoPE of the q|k heads in place, or -- qkn = (q_norm weight, k_norm
    weight, eps), Qwen3 -- per-head RMSNorm + RoPE of q|k into a separate buffer qk (the raw values stay in qkv for backward, v is read
    where it is) with the norms' rstd; qk and rstd are None otherwise."""
    B, S, Hq, Hkv, D, causal, scale = dims
    qk = rstd = None
    if qkn is not None:
        assert cos is not None, "the q/k norm path always applies RoPE"
        qk, rstd = K.qk_norm_rope_fwd(qkv, B * S, Hq, Hkv, D, qkn[0].data, qkn[1].data, qkn[2], cos, sin)
    elif cos is not None and not roped:
        K.rope_apply_(qkv, B * S, Hq + Hkv, D, (Hq + 2 * Hkv) * D, cos, sin)
    out, lse = K.attn_fwd(*qkv_views(qkv if qk is None else qk, B, S, Hq, Hkv, D, v_of=qkv), key_mask, causal, scale)
    return out, lse, qk, rstd


def _rope_attention_backward(dout, qkv, out, lse, cos, sin, key_mask, dims, qkn=None, qk=None, rstd=None):
    """-> dqkv, the gradient of the fused projection output: attention backward, then the RoPE stage's.  Plain: d(q|k) lands in dqkv
    beside dv and is un-roped in place.  qkn = (q_norm weight, k_norm weight) (Qwen3): d(q|k) lands in dqk (qk's strides),
    mm_qk_norm_rope_bwd fills the q|k columns of dqkv from it, and the norm weights' gradients are written."""
    B, S, Hq, Hkv, D, causal, scale = dims
    dqkv = _attn_grad_like(qkv)
    dqk = dqkv if qk is None else _attn_grad_like(qk)
    K.attn_bwd(*qkv_views(qkv if qk is None else qk, B, S, Hq, Hkv, D, v_of=qkv), out, dout.contiguous().view(B, S, Hq, D), lse, key_mask,
               causal, scale, *qkv_views(dqk, B, S, Hq, Hkv, D, v_of=dqkv))
    if qkn is not None:
        qn, kn = qkn
        dwq, dwk = K.qk_norm_rope_bwd(dqk, qkv, B * S, Hq, Hkv, D, qn.data, kn.data, rstd, cos, sin, dqkv,
                                      want_dw=qn.requires_grad or kn.requires_grad)
        _reduce_into(qn, dwq)
        _reduce_into(kn, dwk)
    elif cos is not None:
        K.rope_apply_(dqkv, B * S, Hq + Hkv, D, (Hq + 2 * Hkv) * D, cos, sin, inverse=True)
    return dqkv


class RopeAttentionFn(torch.autograd.Function):
    """qkv [T, (Hq+2Hkv)*D] (fused projection output, consumed in place) -> out [T, Hq*D].
    RoPE (optional) is applied in place to the q and k heads, then flash attention."""

    @staticmethod
    def forward(ctx, qkv, cos, sin, key_mask, B, S, Hq, Hkv, D, causal, scale):
        assert qkv.shape == (B * S, (Hq + 2 * Hkv) * D) and qkv.is_contiguous()
        ctx.dims = (B, S, Hq, Hkv, D, causal, scale)
        out, lse, _, _ = _rope_attention_forward(qkv, cos, sin, key_mask, ctx.dims)
        ctx.save_for_backward(qkv, out, lse, cos, sin, key_mask)
        return out.view(B * S, Hq * D)

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, cos, sin, key_mask = ctx.saved_tensors
        return (_rope_attention_backward(dout, qkv, out, lse, cos, sin, key_mask, ctx.dims),) + (None,) * 10


def rope_attention(qkv, cos, sin, key_mask, B, S, Hq, Hkv, D, causal, scale):
    return RopeAttentionFn.apply(qkv, cos, sin, key_mask, B, S, Hq, Hkv, D, causal, scale)


class QKVRopeAttentionFn(torch.autograd.Function):
    """The decoder's attention front half as ONE node: the fused q|k|v projection, then RopeAttentionFn's two halves.  The projection
    carries RoPE in its epilogue (mm_gemm_rope_fwd) where the shape qualifies and no q/k norm stands in between; the projection +
    the RoPE stage otherwise: same bits.  h [T, H] -> out [T, Hq*D].  Backward = _rope_attention_backward, then the projection's
    (`_proj_backward`: LinearFn's).  qkn: (q_norm weight, k_norm weight, eps) of a Qwen3 layer, see _rope_attention_forward."""

    @staticmethod
    def forward(ctx, h, dummy, wg: ParamGroup, bg: Optional[ParamGroup], cos, sin, key_mask, B, S, Hq, Hkv, D, causal, scale, qkn=None):
        w = wg.tensor()
        b = bg.tensor() if bg is not None else None
        qkv = K.gemm_rope_fwd(h, w, b, (Hq + Hkv) * D, D, cos, sin) if cos is not None and qkn is None else None
        roped = qkv is not None
        if not roped:
            qkv = K.linear_fwd(h, w, bias=b)
        ctx.dims = (B, S, Hq, Hkv, D, causal, scale)
        out, lse, qk, rstd = _rope_attention_forward(qkv, cos, sin, key_mask, ctx.dims, roped, qkn)
        ctx.wg, ctx.bg, ctx.qkn = wg, bg, (qkn[:2] if qkn is not None else None)
        ctx.save_for_backward(h, qkv, out, lse, cos, sin, key_mask, qk, rstd)
        return out.view(B * S, Hq * D)

    @staticmethod
    def backward(ctx, dout):
        h, qkv, out, lse, cos, sin, key_mask, qk, rstd = ctx.saved_tensors
        dqkv = _rope_attention_backward(dout, qkv, out, lse, cos, sin, key_mask, ctx.dims, ctx.qkn, qk, rstd)
        return (_proj_backward(dqkv, h, ctx.wg, ctx.bg, ctx.needs_input_grad[0]),) + (None,) * 14


def qkv_rope_attention(h, wg, bg, cos, sin, key_mask, B, S, Hq, Hkv, D, causal, scale, dummy=None, qkn=None):
    """qkn: optional (q_norm weight, k_norm weight, eps) of a Qwen3 layer (per-head RMSNorm of q and k in front of RoPE)."""
    return QKVRopeAttentionFn.apply(h, dummy, as_group(wg), as_group(bg) if bg is not None else None, cos, sin, key_mask, B, S, Hq, Hkv, D,
                                    causal, scale, qkn)


class HeadPadFn(torch.autograd.Function):
    """[rows, nheads*d] <-> [rows, nheads*dpad]: zero-pad (or strip) every head so that a head width the MFMA attention
    does not tile (SigLIP-so400m: 72) runs on the D = 64 / 128 kernels.  Zero columns add nothing to q.k and give zero
    columns of p.v, so the result is exact; the backward of a pad is a strip and vice versa."""

    @staticmethod
    def forward(ctx, x, nheads, d, dpad, inverse):
        ctx.meta = (nheads, d, dpad, inverse)
        return K.head_pad(x.contiguous(), nheads, d, dpad, inverse)

    @staticmethod
    def backward(ctx, dy):
        nheads, d, dpad, inverse = ctx.meta
        return K.head_pad(dy.contiguous(), nheads, d, dpad, not inverse), None, None, None, None


def head_pad(x, nheads, d, dpad):
    return HeadPadFn.apply(x, nheads, d, dpad, False)


def head_strip(x, nheads, d, dpad):
    return HeadPadFn.apply(x, nheads, d, dpad, True)


def attention_head_width(d: int, dtype) -> int:
    """Head width the attention kernels run a head of width d at (bf16 MFMA path: 64 or 128; fp32 path: any)."""
    if dtype == torch.float32 or d in (64, 128):
        return d
    if d > 128:
        raise ValueError(f"head_dim {d} > 128 is not supported by the bf16 attention kernels")
    return 64 if d < 64 else 128


# Philox streams of the dropout kernels: key = torch's seed (torch.manual_seed governs it), one counter offset per dropout site
# and call; backward regenerates a mask from the (seed, offset) its forward drew.
_dropout_calls = 0


def next_dropout_stream():
    global _dropout_calls
    _dropout_calls += 1
    return int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF, _dropout_calls


class CrossAttentionFn(torch.autograd.Function):
    """Non-causal attention of Nq queries over Nkv keys/values with separate inputs (model/attention.py:79-96 between the
    projections): q2d [n*Nq, h*d], kv2d [n*Nkv, 2*h*d] (k | v, one fused projection output) -> [n*Nq, h*d].
    drop_p > 0: dropout on the attention probabilities (attention.py:40,91).  Up to 1024 keys the one-pass kernel mm_xattn_* runs
    (any head width up to 512: the reference's recipes use 96 and 512); beyond that the flash kernels (d in {64, 128}, no dropout)."""

    @staticmethod
    def forward(ctx, q2d, kv2d, n, Nq, Nkv, heads, d, scale, drop_p):
        C = heads * d
        q = q2d.view(n, Nq, heads, d)
        k = kv2d[:, :C].view(n, Nkv, heads, d)
        v = kv2d[:, C:].view(n, Nkv, heads, d)
        small = K.xattn_supported(q2d.dtype, Nkv, d)
        seed = off = 0
        if small:
            if drop_p > 0.0:
                seed, off = next_dropout_stream()
            out, lse = K.xattn_fwd(q, k, v, scale, drop_p, seed, off)
        else:
            if drop_p > 0.0:
                raise NotImplementedError(f"attention dropout over {Nkv} keys: mm_xattn_* holds a query's scores in registers (<= 1024 keys)")
            out, lse = K.attn_fwd(q, k, v, None, False, scale)
        ctx.dims = (n, Nq, Nkv, heads, d, scale, drop_p, seed, off, small)
        ctx.save_for_backward(q2d, kv2d, out, lse)
        return out.view(n * Nq, C)

    @staticmethod
    def backward(ctx, dout):
        q2d, kv2d, out, lse = ctx.saved_tensors
        n, Nq, Nkv, heads, d, scale, drop_p, seed, off, small = ctx.dims
        C = heads * d
        dq2d, dkv2d = _attn_grad_like(q2d, atomics=not small), _attn_grad_like(kv2d, atomics=not small)    # mm_xattn_bwd: no atomics
        args = (q2d.view(n, Nq, heads, d), kv2d[:, :C].view(n, Nkv, heads, d), kv2d[:, C:].view(n, Nkv, heads, d), out,
                dout.contiguous().view(n, Nq, heads, d), lse)
        grads = (dq2d.view(n, Nq, heads, d), dkv2d[:, :C].view(n, Nkv, heads, d), dkv2d[:, C:].view(n, Nkv, heads, d))
        if small:
            K.xattn_bwd(*args, scale, drop_p, seed, off, *grads)
        else:
            K.attn_bwd(*args, None, False, scale, *grads)
        return dq2d, dkv2d, None, None, None, None, None, None, None


def cross_attention(q2d, kv2d, n, Nq, Nkv, heads, d, scale, drop_p=0.0):
    return CrossAttentionFn.apply(q2d, kv2d, n, Nq, Nkv, heads, d, scale, float(drop_p))


class DropoutFn(torch.autograd.Function):
    """nn.Dropout (attention.py:41,98 `proj_drop`): y = x * keep / (1 - p); the mask is regenerated in backward."""

    @staticmethod
    def forward(ctx, x, p):
        ctx.stream = (p,) + next_dropout_stream()
        return K.dropout(x, *ctx.stream)

    @staticmethod
    def backward(ctx, dy):
        return K.dropout(dy, *ctx.stream), None


def dropout(x, p, training=True):
    return DropoutFn.apply(x, float(p)) if (training and p > 0.0) else x


class ExpertFuseFn(torch.autograd.Function):
    """Gating-weighted fusion of stacked expert features x [E, n, P, C] (image_modality_moe.py:163-205); `gate` [n, E] fp32 is
    the gating network's output.  It receives a gradient (mm_expert_fuse_gate_bwd, fp32) only when it requires one: the experts'
    features are kept for the backward in that case alone."""

    @staticmethod
    def forward(ctx, x, gate, idx, mode):
        E, n, P, C = x.shape
        ctx.meta = (tuple(idx), mode, E, P, C)
        xf = x.reshape(E, n, P * C)
        if gate.requires_grad:
            ctx.save_for_backward(gate, xf if xf.is_contiguous() else xf.contiguous())
        else:
            ctx.save_for_backward(gate)
        out = K.expert_fuse(xf, gate, idx, mode)
        return out.view(n, P, C) if mode == 0 else out.view(n, len(idx) * P, C)

    @staticmethod
    def backward(ctx, dout):
        gate, *kept = ctx.saved_tensors
        idx, mode, E, P, C = ctx.meta
        n = dout.shape[0]
        d = dout.contiguous().view(n, P * C) if mode == 0 else dout.contiguous().view(n, len(idx), P * C)
        dx = K.expert_fuse(d, gate, idx, mode, backward=True, E=E) if ctx.needs_input_grad[0] else None
        dgate = K.expert_fuse_gate_bwd(kept[0], d, gate, idx, mode) if kept and ctx.needs_input_grad[1] else None
        return (dx.view(E, n, P, C) if dx is not None else None), dgate, None, None


def expert_fuse(x, gate, idx, mode):
    return ExpertFuseFn.apply(x, gate, list(idx), mode)


# --------------------------------------------------------------------------------------------------- activations
class SwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu, I):
        ctx.I = I
        ctx.save_for_backward(gu)
        return K.swiglu_fwd(gu, I)

    @staticmethod
    def backward(ctx, dout):
        (gu,) = ctx.saved_tensors
        return K.swiglu_bwd(gu, dout.contiguous(), ctx.I), None


def swiglu(gu, I):
    return SwiGLUFn.apply(gu, I)


class SwiGLUMLPFn(torch.autograd.Function):
    """y = down_proj(silu(gate_proj(x)) * up_proj(x)) + residual as ONE autograd node (HF:llama:163-176 + the residual add of
    :317).  Forward: the SwiGLU is the epilogue of the fused gate|up GEMM (mm_gemm_swiglu_fwd), the residual the epilogue of
    down_proj.  Backward: d(gate|up) comes straight out of down_proj's dgrad GEMM (mm_gemm_swiglu_bwd); d(act) never exists
    in HBM.  Falls back to the separate swiglu kernels when a shape does not qualify (same arithmetic, bit-identical)."""

    @staticmethod
    def forward(ctx, x, residual, dummy, wgu: ParamGroup, wd: ParamGroup, I: int):
        fused = K.gemm_swiglu_fwd(x, wgu.tensor(), I)
        if fused is None:
            gu = K.linear_fwd(x, wgu.tensor())
            act = K.swiglu_fwd(gu, I)
        else:
            gu, act = fused
        y = K.linear_fwd(act, wd.tensor(), residual=residual)
        ctx.wgu, ctx.wd, ctx.I = wgu, wd, I
        ctx.has_res = residual is not None
        ctx.save_for_backward(x, gu, act)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gu, act = ctx.saved_tensors
        wgu, wd, I = ctx.wgu, ctx.wd, ctx.I
        dy = _gemm_rows(dy)
        dres = dy if ctx.has_res else None
        _proj_backward(dy, act, wd, None, False)              # down_proj: the weight gradient first; its dgrad carries the SwiGLU backward
        dgu = K.gemm_swiglu_bwd(dy, wd.tensor(), gu, I)
        if dgu is None:
            dgu = K.swiglu_bwd(gu, K.linear_dgrad(dy, wd.tensor()), I)
        return _proj_backward(dgu, x, wgu, None, ctx.needs_input_grad[0]), dres, None, None, None, None


def swiglu_mlp(x, wgu, wd, I, residual=None, dummy=None):
    return SwiGLUMLPFn.apply(x, residual, dummy, as_group(wgu), as_group(wd), I)


class XIELUMLPFn(torch.autograd.Function):
    """y = down_proj(xIELU(up_proj(x))) + residual as ONE autograd node (HF 5.15 models/apertus ApertusMLP + the layer's residual
    add).  `act` holds the activation's two raw scalars (`alpha_p`, `alpha_n`, Parameters of shape [1]) and `consts()` -> (beta, eps)
    as floats.  Backward: down_proj's wgrad and dgrad, mm_xielu_bwd (dx and the scalar gradients' partial sums in one pass),
    mm_xielu_reduce into the scalars' gradients (overwrite on the first write of a step, accumulate afterwards), up_proj's wgrad and
    dgrad."""

    @staticmethod
    def forward(ctx, x, residual, dummy, wu: ParamGroup, wd: ParamGroup, act):
        beta, eps = act.consts()
        u = K.linear_fwd(x, wu.tensor())
        a = K.xielu_fwd(u, act.alpha_p.data, act.alpha_n.data, beta, eps)
        y = K.linear_fwd(a, wd.tensor(), residual=residual)
        ctx.wu, ctx.wd, ctx.act, ctx.consts = wu, wd, act, (beta, eps)
        ctx.has_res = residual is not None
        ctx.save_for_backward(x, u, a)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, u, a = ctx.saved_tensors
        wu, wd, act = ctx.wu, ctx.wd, ctx.act
        beta, eps = ctx.consts
        dy = _gemm_rows(dy)
        dres = dy if ctx.has_res else None
        da = _proj_backward(dy, a, wd, None, True)
        ap, an = act.alpha_p, act.alpha_n
        train = ap.requires_grad or an.requires_grad
        du, partials = K.xielu_bwd(u, da, ap.data, an.data, beta, eps, want_dalpha=train)
        # one launch writes both scalars' gradients; unlike a LayerNorm's pair they have no one-parameter form
        if train and not _write_grads(K.xielu_reduce, (partials, ap.data, an.data), ap, an):
            raise NotImplementedError("xIELU: alpha_p and alpha_n are trained or frozen together")
        return _proj_backward(du, x, wu, None, ctx.needs_input_grad[0]), dres, None, None, None, None


def xielu_mlp(h, w_up, w_down, act, residual=None, dummy=None):
    return XIELUMLPFn.apply(h, residual, dummy, as_group(w_up), as_group(w_down), act)


class AddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        return K.add(a, b)

    @staticmethod
    def backward(ctx, d):
        return d, d


def add(a, b):
    return AddFn.apply(a, b)


# --------------------------------------------------------------------------------------------------- embed + splice
class EmbedSpliceFn(torch.autograd.Function):
    """model.py:433-444 in one pass: token embedding gather with modality rows spliced in."""

    @staticmethod
    def forward(ctx, proj, dummy, emb, ids, batch_idx, token_range, B, S, padding_idx=None):
        ctx.padding_idx = padding_idx
        T = B * S
        ids = ids.reshape(-1).contiguous()
        src_map = None
        if proj is not None:
            src_map = K.splice_build_map(batch_idx, token_range, S, T)
            proj = proj.reshape(-1, proj.shape[-1])
            if proj.dtype != emb.dtype:   # model.py:443-444 casts the modality rows to the embedding dtype
                proj = K.cast(proj, emb.dtype)
            proj = proj.contiguous()
        out = K.embed_splice_fwd(emb.data, ids, proj, src_map)
        order = skey = None
        if emb.requires_grad and torch.is_grad_enabled():
            # the embedding gradient's summation order (a stable sort of the tokens by id) depends on ids and the splice
            # map only: built here, beside the forward, instead of at the tail of backward
            order, skey = K.embed_sort(ids, src_map, emb.shape[0], emb.shape[1])
        ctx.emb = emb
        ctx.S = S
        ctx.has_proj = proj is not None
        ctx.proj_rows = proj.shape[0] if proj is not None else 0
        ctx.save_for_backward(ids, src_map, batch_idx, token_range, order, skey)
        return out

    @staticmethod
    def backward(ctx, dE):
        ids, src_map, batch_idx, token_range, order, skey = ctx.saved_tensors
        emb = ctx.emb
        dE = dE.contiguous()
        if _defer is not None and _defer["items"]:      # the decoder's backward is done: release the held-back wgrads
            _defer["event"] = flush_deferred_wgrads()
        dproj = None
        if ctx.has_proj and ctx.needs_input_grad[0]:
            dproj = torch.empty((ctx.proj_rows, dE.shape[1]), dtype=dE.dtype, device=dE.device)
        demb = None
        acc = False
        if emb.requires_grad:
            demb, acc = grad_target(emb)
            if order is None:          # forward ran under no_grad bookkeeping (e.g. requires_grad flipped afterwards)
                order, skey = K.embed_sort(ids, src_map, emb.shape[0], emb.shape[1])
            if not acc:
                demb.zero_()           # rows no token touched must read 0 (the flat gradient buffer is never memset)
        K.embed_splice_bwd(dE, ids, src_map, batch_idx, token_range, ctx.S, dproj, demb, order, skey, accumulate=acc)
        if emb.requires_grad:
            if ctx.padding_idx is not None:      # nn.Embedding(padding_idx=...): that row never receives a gradient
                demb[ctx.padding_idx].zero_()
            _ready(emb)
        return dproj, None, None, None, None, None, None, None, None


def embed_splice(emb, ids, proj, batch_idx, token_range, B, S, dummy=None, padding_idx=None):
    return EmbedSpliceFn.apply(proj, dummy, emb, ids, batch_idx, token_range, B, S, padding_idx)


# --------------------------------------------------------------------------------------------------- ViT glue
class PatchEmbedFn(torch.autograd.Function):
    """conv(k=s=patch) as patchify + GEMM, then positions.  CLIP (HF:clip:138-218): no conv bias, CLS row prepended.
    SigLIP (HF:siglip SiglipVisionEmbeddings): conv bias, no CLS row (cls is None)."""

    @staticmethod
    def forward(ctx, pixels, dummy, w_conv, b_conv, cls, pos, ps):
        n = pixels.shape[0]
        Dv = w_conv.shape[0]
        kk = 3 * ps * ps
        kpad = (kk + 63) // 64 * 64
        dtype = w_conv.dtype
        patches = K.patchify(pixels.contiguous(), ps, kpad, dtype)
        wp = torch.zeros((Dv, kpad), dtype=dtype, device=w_conv.device)
        wp[:, :kk].copy_(w_conv.data.reshape(Dv, kk))
        po = K.linear_fwd(patches, wp, bias=b_conv.data if b_conv is not None else None)
        P = patches.shape[0] // n
        if cls is not None:
            x = K.vit_embed_fwd(po, cls.data, pos.data, n, P)
            T = P + 1
        else:
            x = K.bcast_add(po.view(n, P * Dv), pos.data.reshape(-1))
            T = P
        ctx.params = (w_conv, b_conv, cls, pos)
        ctx.meta = (n, P, Dv, kk, kpad)
        ctx.save_for_backward(patches)
        return x.view(n * T, Dv)

    @staticmethod
    def backward(ctx, dx):
        (patches,) = ctx.saved_tensors
        w_conv, b_conv, cls, pos = ctx.params
        n, P, Dv, kk, kpad = ctx.meta
        need_w = w_conv.requires_grad
        need_b = b_conv is not None and b_conv.requires_grad
        gc = gp = None
        accc = accp = False
        if cls is not None and cls.requires_grad:
            gc, accc = grad_target(cls)
        if pos.requires_grad:
            gp, accp = grad_target(pos)
        if not (need_w or need_b or gc is not None or gp is not None):
            return (None,) * 7
        if cls is not None:
            dx = dx.contiguous().view(n, P + 1, Dv)
            if gc is not None and gp is not None and accc != accp:   # kernel takes one flag: normalise by zeroing
                (gc if not accc else gp).zero_()
                accc = accp = True
            dpatch = K.vit_embed_bwd(dx, gc, gp, accc or accp, want_dpatch=need_w or need_b)
        else:
            dpatch = dx.contiguous().view(n * P, Dv)                 # no CLS row: the patch gradient IS dx
            if gp is not None:
                K.colsum(dpatch.view(n, P * Dv), gp.view(-1), accp)
        if need_b:
            _write_grads(K.colsum, (dpatch,), b_conv)
        if need_w:      # the GEMM runs on the K-padded patches: into a padded buffer, whose first kk columns then reach the filter's gradient
            gw = torch.empty((Dv, kpad), dtype=dx.dtype, device=dx.device)
            K.linear_wgrad(dpatch, patches, gw, False)
            g, acc = grad_target(w_conv)          # not _write_grads: torch's add_ / copy_ stand where a kernel would
            if acc:
                g.add_(gw[:, :kk].reshape(g.shape))
            else:
                g.copy_(gw[:, :kk].reshape(g.shape))
            _ready(w_conv)
        for p in (cls, pos):
            if p is not None and p.requires_grad:
                _ready(p)
        return (None,) * 7


def patch_embed(pixels, w_conv, cls, pos, ps, dummy=None, b_conv=None):
    return PatchEmbedFn.apply(pixels, dummy, w_conv, b_conv, cls, pos, ps)


class DropClsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, n, T):
        return K.drop_cls_fwd(x.view(n, T, -1))

    @staticmethod
    def backward(ctx, dy):
        d = K.drop_cls_bwd(dy.contiguous())
        return d.view(-1, d.shape[-1]), None, None


def drop_cls(x, n, T):
    return DropClsFn.apply(x, n, T)


# --------------------------------------------------------------------------------------------------- loss
class CausalLMLossFn(torch.autograd.Function):
    """HF:loss/loss_utils.py:36-71 on the (padded-stride) logits: mean CE over labels != -100, labels pre-shifted."""

    @staticmethod
    def forward(ctx, logits2d, V, shift_labels):
        lc, lse = K.ce_fwd(logits2d, V, shift_labels)
        ctx.V = V
        ctx.save_for_backward(logits2d, shift_labels, lse, lc)
        return lc[0].clone()

    @staticmethod
    def backward(ctx, dloss):
        logits2d, labels, lse, lc = ctx.saved_tensors
        T = logits2d.shape[0]
        ld = logits2d.stride(0)
        buf = torch.empty((T, ld), dtype=logits2d.dtype, device=logits2d.device)
        d = buf[:, : logits2d.shape[1]]
        g = dloss.reshape(1).to(torch.float32).contiguous()
        K.ce_bwd(logits2d, ctx.V, labels, lse, lc, g, d)
        return d, None, None


class LossRows:
    """The rows of a [B*S] batch whose SHIFTED label is not -100, as the host knows them (built where the labels still are a
    host tensor: train/prefetch.py, or CausalLM.forward for host labels): `idx` int32 [n] ascending, `inv` int32 [B*S] (-1 at
    ignored rows), `labels` int64 [n] (the shifted labels of those rows), all on the device."""
    __slots__ = ("idx", "inv", "labels", "n", "total")

    def __init__(self, idx, inv, labels, n, total):
        self.idx, self.inv, self.labels, self.n, self.total = idx, inv, labels, int(n), int(total)

    @staticmethod
    def host_parts(labels_host: torch.Tensor):
        """-> (idx int32 [n], inv int32 [B*S], shifted labels int64 [n]) on the host; HF:loss/loss_utils.py:52-56 shift."""
        shift = torch.nn.functional.pad(labels_host, (0, 1), value=-100)[..., 1:].reshape(-1)
        keep = shift != -100
        idx = torch.nonzero(keep).reshape(-1).to(torch.int32)
        inv = torch.full((shift.numel(),), -1, dtype=torch.int32)
        inv[keep] = torch.arange(idx.numel(), dtype=torch.int32)
        return idx, inv, shift[keep].contiguous()

    @classmethod
    def from_host_labels(cls, labels_host, device):
        idx, inv, lab = cls.host_parts(labels_host)
        return cls(idx.to(device), inv.to(device), lab.to(device), idx.numel(), inv.numel())


class RowsSelectFn(torch.autograd.Function):
    """y = x[rows.idx]; backward scatters dy back into a [B*S, H] gradient with exact zeros at the ignored rows."""

    @staticmethod
    def forward(ctx, x2d, rows):
        ctx.rows = rows
        return K.rows_select(x2d, rows.idx, rows.n)

    @staticmethod
    def backward(ctx, dy):
        rows = ctx.rows
        return K.rows_select(dy.contiguous(), rows.inv, rows.total), None


def rows_select(x2d, rows):
    return RowsSelectFn.apply(x2d, rows)


def causal_lm_loss(logits2d, V, shift_labels):
    return CausalLMLossFn.apply(logits2d, V, shift_labels)
