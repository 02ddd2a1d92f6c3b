"""How the E expert towers of the MoE image modalities run (modalities/image_modality_moe.py calls `run_experts`).  E towers are E
launch-latency-bound chains of short kernels, bounded by the HOST; five paths, the same kernels and the same bits on each:

    grouped        ONE chain of grouped launches, the expert as a batch dimension (model/vision_grouped.py): ordinary autograd, no
                   graph, no side stream, no state between calls.  Opt-in (config `grouped_towers`, MM_MOE_GROUPED), for eligible
                   experts: one VisionConfig, one dtype, all on the device, at most MM_GROUP_MAX of them; others warn once and go on
    frozen_graph   frozen towers (the shipped alignment / end2end recipes; also any no-grad call): one captured hipGraph per pixel
                   shape, the towers on parallel branches; a replay costs the host nothing (`_frozen_towers`; MM_MOE_GRAPH=0: off)
    train_graph    trainable towers whose gradients live in a flat buffer: captured forward and backward graphs (`_TowerGraphs`,
                   `_trainable_towers`; MM_MOE_TRAIN_GRAPH=0: off)
    streams        eager launches, each tower on ITS OWN HIP stream: E side by side take little more than one; autograd replays each
                   tower's backward on the stream its forward ran on (MM_MOE_STREAMS=0: off)
    serial         eager launches, one tower after the other on the current stream

`choose_path` is the table that picks one: plain facts in, a name out (tests/test_expert_towers_cpu.py).  The graph runners keep
their graphs in `experts._mm_graphs`; the side streams (`_expert_stream`) are one process-wide table."""
from __future__ import annotations

import os
import warnings

import torch

from .. import functional as Fm
from ..nn import fire_forward_pre_hooks, grad_dummy
from . import vision_grouped


def _grouped_on(grouped) -> bool:
    """the `grouped_towers` switch: the config field, overridden by MM_MOE_GROUPED=0|1"""
    env = os.environ.get("MM_MOE_GROUPED")
    return bool(grouped) if env in (None, "") else env != "0"


def _switches():
    """MM_MOE_GRAPH, MM_MOE_TRAIN_GRAPH, MM_MOE_STREAMS ("0" = off), read on every call: tests and tools/moe_bench.py flip them"""
    return tuple(os.environ.get(k, "1") for k in ("MM_MOE_GRAPH", "MM_MOE_TRAIN_GRAPH", "MM_MOE_STREAMS"))


_warned_ineligible = False


def eager_path(n_experts, on_device, streams="1"):
    """rule 4 of `choose_path`: also what a call takes that the trainable towers' graphs decline"""
    return "serial" if n_experts == 1 or not on_device or streams == "0" else "streams"


def choose_path(grouped_on, ineligible, on_device, frozen, pixels_need_grad, graphable, n_experts, graph="1", train_graph="1", streams="1"):
    """-> "grouped" | "frozen_graph" | "train_graph" | "streams" | "serial"; top to bottom, the first match wins.
    `ineligible` (-> None, or why the experts cannot run grouped), `frozen` and `graphable` are called only when the table gets to
    them: `ineligible` only with the switch on, `frozen` (a walk over every parameter) not on the grouped path."""
    if grouped_on:
        why = ineligible()
        if why is None:
            return "grouped"
        global _warned_ineligible
        if not _warned_ineligible:
            _warned_ineligible = True
            warnings.warn(f"grouped_towers: {why}; the expert towers run one by one")
    is_frozen = frozen()
    if is_frozen and on_device and graph != "0":
        return "frozen_graph"
    if not is_frozen and on_device and not pixels_need_grad and graph != "0" and train_graph != "0" and graphable():
        return "train_graph"
    return eager_path(n_experts, on_device, streams)


def run_experts(experts, pixels, post=None, grouped=False):
    """Every expert tower on the same pixels (reference image_modality_moe.py:156-160) -> E token tensors [n, P, C], each through
    `post(e, tokens)` when given (the per-expert projectors: trainable, so outside any graph).  `grouped`: the config field
    `grouped_towers`.  The path is `choose_path`'s; same kernels on each, same results bit for bit."""
    n = pixels.shape[0]

    def tower(e, expert, px=None):
        hs = expert(pixels if px is None else px).last_hidden_state                             # [n, 1+P, C]
        T = hs.shape[1]
        return Fm.drop_cls(hs.reshape(n * T, -1), n, T)                                          # [n, P, C]

    graph, train_graph, streams = _switches()
    path = choose_path(_grouped_on(grouped),
                       lambda: vision_grouped.ineligible(experts) if pixels.is_cuda else "the pixels are not on the device",
                       pixels.is_cuda,
                       lambda: not torch.is_grad_enabled() or not any(p.requires_grad for ex in experts for p in ex.parameters()),
                       pixels.requires_grad, lambda: _graphable(experts), len(experts), graph, train_graph, streams)
    if path == "grouped":
        outs = vision_grouped.grouped_towers(experts, pixels)
    elif path == "frozen_graph":
        outs = _frozen_towers(experts, pixels, tower)
    elif path == "train_graph":
        outs = _trainable_towers(experts, pixels, tower)
        if outs is None:
            # declined: a forward of this pixel shape still waits for its backward (two micro-batch losses summed before .backward(),
            # a grad-enabled evaluation in between): the graphs' saved activations are shared buffers, so THIS call runs eagerly
            path = eager_path(len(experts), pixels.is_cuda, streams)
    if path == "streams":
        return _stream_towers(experts, pixels, tower, post)
    if path == "serial":
        outs = (tower(e, ex) for e, ex in enumerate(experts))            # lazily: `post` follows each tower at once, as the launches always went
    return list(outs) if post is None else [post(e, o) for e, o in enumerate(outs)]


def _stream_towers(experts, pixels, tower, post):
    """each tower, and its `post`, on the expert's own stream: `post` must have run there before record_stream"""
    main = torch.cuda.current_stream()
    outs = []
    for e, ex in enumerate(experts):
        st = _expert_stream(pixels.device, e)
        st.wait_stream(main)                                              # pixels (and the previous step's work) are ready
        with torch.cuda.stream(st):
            o = tower(e, ex)
            if post is not None:
                o = post(e, o)
        o.record_stream(main)                                             # produced on `st`, consumed on the compute stream
        outs.append((o, st))
    for _, st in outs:
        main.wait_stream(st)
    return [o for o, _ in outs]


def _frozen_towers(experts, pixels, tower):
    """Captured-graph forward of frozen expert towers: -> list of [n, P, C] token tensors (no autograd history).  One graph per
    (image count, image size, parameter storage); the pixels are copied into the graph's input buffer, the outputs out of its pool."""
    key = (tuple(pixels.shape), pixels.dtype, experts[0].embeddings.position_embedding.weight.data_ptr())
    cache = getattr(experts, "_mm_graphs", None)
    if cache is None:
        cache = experts._mm_graphs = {}
    ent = cache.get(key)
    if ent is None:
        with torch.no_grad():
            static_px = pixels.clone()
            cur = torch.cuda.current_stream()
            warm = torch.cuda.Stream()
            warm.wait_stream(cur)
            with torch.cuda.stream(warm):                                 # lazy initialisation (kernel attributes, id checks) outside capture
                for _ in range(2):
                    for e, ex in enumerate(experts):
                        tower(e, ex, static_px)
            cur.wait_stream(warm)
            graph = torch.cuda.CUDAGraph()
            with _no_gc(), torch.cuda.graph(graph):
                main = torch.cuda.current_stream()
                res = []
                for e, ex in enumerate(experts):                          # fork: every tower on its own branch of the graph
                    st = _expert_stream(pixels.device, e)
                    st.wait_stream(main)
                    with torch.cuda.stream(st):
                        res.append(tower(e, ex, static_px))
                for e in range(len(experts)):
                    main.wait_stream(_expert_stream(pixels.device, e))    # join
        ent = cache[key] = (graph, static_px, res)
        if len(cache) > 8:                                                # a handful of image counts at most: drop the oldest
            cache.pop(next(iter(cache)))
    graph, static_px, res = ent
    static_px.copy_(pixels)
    graph.replay()
    return [o.clone() for o in res]


class _no_gc:
    """No automatic garbage collection while a hipGraph is being captured: a collection that happens to run mid-capture can destroy
    an OLDER graph (an earlier model's towers) -- releasing a graph's memory pool is not a capturable operation and aborts the
    process.  (torch.cuda.graph collects once on entry; this keeps the interpreter from collecting again before the capture ends.)"""

    def __enter__(self):
        import gc
        self.was = gc.isenabled()
        gc.disable()

    def __exit__(self, *exc):
        import gc
        if self.was:
            gc.enable()


def _graphable(experts):
    """Trainable towers can be replayed from captured graphs when every parameter's gradient lives in a flat buffer (the wgrad
    kernels write `param.grad` in place: a gradient tensor allocated during capture would belong to the graph's pool)."""
    return all(getattr(p, "_mm_flat", None) is not None for ex in experts for p in ex.parameters() if p.requires_grad)


class _TowerGraphs:
    """Forward and backward hipGraphs of E TRAINABLE expert towers for one pixel shape.  The forward graph is captured with
    autograd recording, on E parallel branches; the autograd graph of that capture is kept, and the backward graphs are captured
    by running it (per expert, on the expert's branch) -- one graph for `first gradient of the step` (the wgrad kernels overwrite)
    and one for `accumulate`.  A replay costs the host two calls instead of ~1,200 launches per ViT-L/14 tower, which is what
    bounds E trainable towers otherwise (E host-bound chains)."""

    def __init__(self, experts, pixels, tower):
        from .. import functional as F_
        import gc
        torch.cuda.synchronize()            # garbage (older graphs, their pools) goes now, at a quiet point, not in the middle of the
        gc.collect()                        # warm-up / capture / first replay below
        self.experts = experts
        self.params = [p for ex in experts for p in ex.parameters() if p.requires_grad]
        dev = pixels.device
        self.streams = [_expert_stream(dev, e) for e in range(len(experts))]
        self.static_px = pixels.detach().clone()
        cur = torch.cuda.current_stream()
        warm = torch.cuda.Stream()
        warm.wait_stream(cur)
        with torch.cuda.stream(warm), torch.no_grad():                      # lazy initialisation outside capture
            for e, ex in enumerate(experts):
                tower(e, ex, self.static_px)
        cur.wait_stream(warm)
        self.fwd = torch.cuda.CUDAGraph()
        with _no_gc(), torch.enable_grad(), torch.cuda.graph(self.fwd):
            main = torch.cuda.current_stream()
            self.res = []
            for e, ex in enumerate(experts):
                st = self.streams[e]
                st.wait_stream(main)
                with torch.cuda.stream(st):
                    self.res.append(tower(e, ex, self.static_px))
            for st in self.streams:
                main.wait_stream(st)
        self.pool = self.fwd.pool()
        self.static_g = [torch.zeros_like(o) for o in self.res]
        self.bwd = {}
        self.warmed = False
        self._F = F_
        # The saved activations of the capture are SHARED buffers: a second forward before the first one's backward would overwrite
        # what that backward reads, and a second backward of one forward would re-read buffers a later forward has refilled.
        # `generation` counts forwards; `pending` = the generation whose backward has not run yet (None: the buffers are free).
        self.generation = 0
        self.pending = None

    def _flags(self, fresh):
        for p in self.params:
            p._mm_flat.ensure_grad()
            p.grad = p._mm_grad_view
            p._mm_fresh = fresh

    def _run_autograd(self):
        main = torch.cuda.current_stream()
        for e, st in enumerate(self.streams):
            st.wait_stream(main)
            with torch.cuda.stream(st):
                torch.autograd.backward([self.res[e]], [self.static_g[e]], retain_graph=True)
        for st in self.streams:
            main.wait_stream(st)

    def forward(self, pixels):
        for ex in self.experts:                  # parameter-read hooks (the Trainer's per-block wait for the overlapped optimiser), looked
            fire_forward_pre_hooks(ex)           # up per call (a Trainer may come later): the replay calls no module
        self.static_px.copy_(pixels)
        self.fwd.replay()
        self.generation += 1
        self.pending = self.generation
        return [o.detach().clone() for o in self.res]

    def backward(self, grads, generation=None):
        if generation is not None and generation != self.pending:
            raise RuntimeError("MoE expert towers (graph replay): backward of a forward whose saved activations are gone -- it ran "
                               "twice, or another forward of the same pixel shape ran in between (MM_MOE_TRAIN_GRAPH=0 = eager towers)")
        self.pending = None
        F_ = self._F
        p0 = self.params[0]
        fresh = p0.grad is None or bool(getattr(p0, "_mm_fresh", False))
        for sg, g in zip(self.static_g, grads):
            if g is None:
                sg.zero_()
            else:
                sg.copy_(g)
        if not self.warmed:                 # first backward: eager, through the autograd graph of the capture (its saved tensors are
            self.warmed = True              # the graph's buffers, which the forward replay has just filled) -- a real backward
            self._flags(fresh)
            hook, order = F_._grad_ready_hook, []

            def spy(p):                     # which parameters report a finished gradient, and in which order: replays repeat it
                order.append(p)
                if hook is not None:
                    hook(p)

            F_.set_grad_ready_hook(spy)
            try:
                self._run_autograd()
            finally:
                F_.set_grad_ready_hook(hook)
            self.ready_order = order
            return
        g = self.bwd.get(fresh)
        if g is None:
            hook = F_._grad_ready_hook
            F_.set_grad_ready_hook(None)    # python side effects do not replay: the hooks are called after every replay instead
            try:
                self._flags(fresh)
                g = torch.cuda.CUDAGraph()
                with _no_gc(), torch.cuda.graph(g, pool=self.pool):
                    self._run_autograd()
            finally:
                F_.set_grad_ready_hook(hook)
            self.bwd[fresh] = g
        self._flags(False)                  # what grad_target leaves behind: .grad attached, the next write accumulates
        g.replay()
        for p in self.ready_order:
            F_._ready(p)


class _TrainableTowersFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dummy, pixels, graphs):
        ctx.graphs = graphs
        out = tuple(graphs.forward(pixels))
        ctx.generation = graphs.generation
        return out

    @staticmethod
    def backward(ctx, *grads):
        ctx.graphs.backward(grads, ctx.generation)
        return None, None, None


def _trainable_towers(experts, pixels, tower):
    """Graph-replayed forward + backward of trainable expert towers (see _TowerGraphs); same kernels as the eager path."""
    key = ("train", tuple(pixels.shape), pixels.dtype, experts[0].embeddings.position_embedding.weight.data_ptr(),
           tuple(p.requires_grad for ex in experts for p in ex.parameters()))
    cache = getattr(experts, "_mm_graphs", None)
    if cache is None:
        cache = experts._mm_graphs = {}
    ent = cache.get(key)
    if ent is None:
        ent = cache[key] = _TowerGraphs(experts, pixels, tower)
        if len(cache) > 8:
            cache.pop(next(iter(cache)))
    if ent.pending is not None:
        return None                          # its buffers hold a forward that still waits for its backward: this call runs eagerly
    p0 = ent.params[0]
    return list(_TrainableTowersFn.apply(grad_dummy(p0), pixels, ent))


_EXPERT_STREAMS = {}


def _expert_stream(device, e):
    key = (device.index or 0, e)
    if key not in _EXPERT_STREAMS:
        _EXPERT_STREAMS[key] = torch.cuda.Stream(device=device)
    return _EXPERT_STREAMS[key]
