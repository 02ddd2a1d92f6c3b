"""Kernel contract of the optimizer kernels (csrc/mm_optim.hip) through the C ABI: m, v and the master weight of every AdamW
entry against fp64 per element (tests/optim_check.py), the parameter and the (bf16, remainder) split bit for bit, the gradient
norm per block, and the refusals by return code with nothing written.  Every output lives in a NaN-sentinel storage (Guarded);
inputs the contract says are not read hold sentinels (clip[0], the parameter of the non-split entries, everything behind n)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from tests import optim_check as OC
from tests.kernel_check import SENTINEL, Guarded, check_bits, dt, options, rc, sentinel_fill
from tests.kernel_check import ptr as p_
from tests.optim_check import BF, F32, Hyper

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ["bf16", "f32", "split"]
ADAMW_N = [1, 3, 4, 5, 1023, 1024, 1027, 100003]
HYPER = {                          # (lr, b1, b2, eps, wd), steps (chained: each call reads what the one before wrote)
    "chained": ((1e-2, 0.9, 0.95, 1e-8, 0.01), [1, 2, 3]),
    "small_lr": ((1e-5, 0.9, 0.999, 1e-8, 0.1), [1, 2, 3, 1000, 100000]),
    "eps": ((1e-3, 0.9, 0.999, 1e-3, 0.0), [2]),             # with |g| about 1e-3: eps is comparable to the root
    "no_decay": ((1e-2, 0.9, 0.95, 1e-8, 0.0), [1]),
}
CLIP = {"null": None, "bites": 0.37, "idle": 1.0}
SUMSQ_N = {BF: [0, 1, 7, 8, 9, 8192, 10245, 100003], F32: [0, 1, 3, 4, 5, 4096, 5125, 100003]}
SUMSQ_NBLK = [1, 2, 1024]
FINISH_NBLK = [1, 255, 256, 257, 3000]
MAX_NORMS = [0.0, -1.0, 1.0, 1e6]
SPLIT_N = [1, 255, 256, 257, 4096 * 256 + 1]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def sync():
    torch.cuda.synchronize()


def f(x):
    return ctypes.c_float(x)


def ids(v):
    return OC.NAME[v] if isinstance(v, torch.dtype) else None


def input_storage(x, off=0, pad=64):
    """x behind `off` and in front of `pad` sentinel elements (nothing outside x is read)"""
    n = x.numel()
    if x.dtype == torch.int16:                                  # a remainder: the bf16 sentinel's bits
        buf = torch.full((off + n + pad,), SENTINEL[BF], dtype=torch.int16, device=DEV)
    else:
        buf = sentinel_fill(torch.empty(off + n + pad, dtype=x.dtype, device=DEV))
    buf[off:off + n] = x
    return buf[off:off + n]


def i16_storage(n, off=0):
    """an int16 output: a guarded bf16 storage seen as int16"""
    g = Guarded(n + off, BF, DEV)
    return g.view((n,), (1,), off).view(torch.int16), g


def bands_intact(name, g):
    """the guard bands alone.  An int16 remainder may take the sentinel's bit pattern, so `never written` cannot be asked of it."""
    iv = g.buf.view(torch.int16 if g.dtype == BF else torch.int32)
    bad = ~g.covered & (iv != SENTINEL[g.dtype])
    assert not bool(bad.any()), f"{name}: write outside the output ({int(bad.sum())} elements)"


def bits_of(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).clone()


# ---- AdamW ---------------------------------------------------------------------------------------------------------------------
class State:
    """the operands of one AdamW entry in guarded storages.  off: elements in front of p, g and lo (the split entry's 8-byte rule)."""

    def __init__(self, kind, pr, ties=False, off=0):
        self.kind, self.n = kind, pr["g"].numel()
        n, self.T = self.n, F32 if kind == "f32" else BF
        self.guards = {}
        self.g = input_storage(pr["g"], off)
        self.m = self._out("m", F32, pr["m"])
        self.v = self._out("v", F32, pr["v"])
        if kind == "split":
            p, lo = OC.split_reference(pr["w"])
            if ties:
                OC.plant_ties(p, lo, 2 * pr["k"], min(pr["k"], 4))
            self.p = self._out("p", BF, p, off)
            self.lo, self.guards["lo"] = i16_storage(n, off)
            self.lo.copy_(lo)
        else:
            self.master = self._out("master", F32, pr["w"])
            self.guards["p"] = Guarded(n, self.T, DEV)          # written, never read: it starts as sentinels
            self.p = self.guards["p"].view((n,), (1,))

    def _out(self, name, dtype, src, off=0):
        self.guards[name] = Guarded(self.n + off, dtype, DEV)
        v = self.guards[name].view((self.n,), (1,), off)
        v.copy_(src)
        return v

    def w(self):
        return OC.join_reference(self.p, self.lo) if self.kind == "split" else self.master.clone()

    def before(self):
        return {"g": self.g, "m": self.m.clone(), "v": self.v.clone(), "w": self.w()}

    def after(self):
        out = {"m": self.m, "v": self.v, "p": self.p}
        out.update({"lo": self.lo} if self.kind == "split" else {"master": self.master})
        return out

    def call(self, h, step, clip, n=None, **ptrs):
        a = {k: p_(getattr(self, k)) for k in ("p", "g", "m", "v") + (("lo",) if self.kind == "split" else ("master",))}
        a.update(ptrs)
        n = self.n if n is None else n
        if self.kind == "split":
            return rc("mm_adamw_step_split", a["p"], a["g"], a["lo"], a["m"], a["v"], n, *h.args(), step, p_(clip))
        return rc("mm_adamw_step", dt(self.T), a["p"], a["g"], a["master"], a["m"], a["v"], n, *h.args(), step, p_(clip))

    def verify(self, tag):
        sync()
        for name, g in self.guards.items():
            if name == "lo":
                bands_intact(f"{tag} lo", g)
            else:
                g.verify(f"{tag} {name}")

    def snapshot(self):
        return {k: bits_of(g.buf) for k, g in self.guards.items()}

    def unchanged(self, snap, tag):
        sync()
        for k, g in self.guards.items():
            assert bool((bits_of(g.buf) == snap[k]).all()), f"{tag}: {k} was written"


def clip_tensor(c):
    if c is None:
        return None
    t = sentinel_fill(torch.empty(2, dtype=F32, device=DEV))       # clip[0], the norm, is not read
    t[1] = c
    return t


def run_adamw(kind, n, hyper, clip, seed):
    hp, steps = HYPER[hyper]
    h = Hyper(*hp)
    pr = OC.adamw_problem(n, F32 if kind == "f32" else BF, DEV, seed, gscale=1e-3 if hyper == "eps" else 1.0)
    st = State(kind, pr, ties=(h.wd == 0))
    ct = clip_tensor(CLIP[clip])
    c = 1.0 if ct is None else float(ct[1])
    for step in steps:
        tag = f"adamw {kind} n={n} {hyper} step={step} clip={clip}"
        before = st.before()
        assert st.call(h, step, ct) == OC.OK, tag
        st.verify(tag)
        OC.check_adamw(tag, before, st.after(), h, step, c, kind)
    return st


@pytest.mark.parametrize("n", ADAMW_N)
@pytest.mark.parametrize("kind", KINDS)
def test_adamw_sizes(kind, n):
    run_adamw(kind, n, "chained", "bites", seed=n)


@pytest.mark.parametrize("kind", KINDS)
def test_adamw_grid_stride(kind):
    with options(adamw_blocks=2):                               # 2501 vectors over 512 threads: five trips
        run_adamw(kind, 10007, "chained", "bites", seed=7)


@pytest.mark.parametrize("clip", list(CLIP))
@pytest.mark.parametrize("hyper", list(HYPER))
@pytest.mark.parametrize("kind", KINDS)
def test_adamw_hyper_parameters(kind, hyper, clip):
    for n in (5, 1027):
        run_adamw(kind, n, hyper, clip, seed=11 + n)


def test_adamw_split_pointers_need_8_bytes_only():
    h = Hyper(*HYPER["chained"][0])
    st = State("split", OC.adamw_problem(1027, BF, DEV, 5), off=4)
    assert st.p.data_ptr() % 16 == 8 and st.g.data_ptr() % 16 == 8 and st.lo.data_ptr() % 16 == 8
    before = st.before()
    assert st.call(h, 1, None) == OC.OK
    st.verify("split at 8-byte offsets")
    OC.check_adamw("split at 8-byte offsets", before, st.after(), h, 1, 1.0, "split")


@pytest.mark.parametrize("kind", KINDS)
def test_adamw_refusals(kind):
    h = Hyper(*HYPER["chained"][0])
    st = State(kind, OC.adamw_problem(1027, F32 if kind == "f32" else BF, DEV, 3))
    snap = st.snapshot()
    names = ("p", "g", "m", "v") + (("lo",) if kind == "split" else ("master",))
    assert st.call(h, 1, None, n=0) == OC.OK
    st.unchanged(snap, "n = 0")
    assert st.call(h, 0, None) == OC.ERR_ARG
    assert st.call(h, 1, None, n=-1) == OC.ERR_ARG
    for k in names:
        assert st.call(h, 1, None, **{k: None}) == OC.ERR_ARG, k
        assert st.call(h, 1, None, n=1023, **{k: p_(getattr(st, k)) + 4}) == OC.ERR_ALIGN, k
    if kind == "split":
        for k in ("m", "v"):
            assert st.call(h, 1, None, n=1023, **{k: p_(getattr(st, k)) + 8}) == OC.ERR_ALIGN, k
    else:
        for k in names:
            assert st.call(h, 1, None, n=1023, **{k: p_(getattr(st, k)) + 8}) == OC.ERR_ALIGN, k
    st.unchanged(snap, "refusals")


def nt0_child():
    """run in a fresh process with MM_ADAMW_NT=0 (the library reads it once): the plain-load instantiations of both bf16 entries"""
    assert os.environ.get("MM_ADAMW_NT") == "0"
    for kind in ("bf16", "split"):
        for n in (5, 1027):
            run_adamw(kind, n, "chained", "bites", seed=n)
        with options(adamw_blocks=2):
            run_adamw(kind, 10007, "chained", "bites", seed=7)
    sync()


def test_adamw_without_nontemporal_access():
    env = dict(os.environ, MM_ADAMW_NT="0")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c",
                        "from tests import test_optim_contract_gpu as t; t.nt0_child()"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"child exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"


# ---- gradient norm -------------------------------------------------------------------------------------------------------------
def partial_call(g, n, nblk):
    part = Guarded(nblk, F32, DEV)
    pv = part.view((nblk,), (1,))
    gptr = p_(g) if n else g.untyped_storage().data_ptr()      # an empty view has no address of its own
    assert rc("mm_gradnorm_partial", dt(g.dtype), gptr, n, p_(pv), nblk) == OC.OK
    sync()
    part.verify(f"partial n={n} nblk={nblk}")
    return pv


def finish_call(part, max_norm):
    gt = Guarded(2, F32, DEV)
    total = gt.view((2,), (1,))
    assert rc("mm_gradnorm_finish", p_(part), part.numel(), f(max_norm), p_(total)) == OC.OK
    sync()
    gt.verify(f"total nblk={part.numel()}")
    return total


@pytest.mark.parametrize("nblk", SUMSQ_NBLK)
@pytest.mark.parametrize("dtype", [BF, F32], ids=ids)
def test_gradnorm(dtype, nblk):
    for n in SUMSQ_N[dtype]:
        for exact in (False, True):
            x, q = OC.sumsq_exact_problem(n, dtype, DEV, n) if exact else (OC.sumsq_problem(n, dtype, DEV, n), None)
            g = input_storage(x)
            tag = f"gradnorm {OC.NAME[dtype]} n={n} nblk={nblk} {'exact' if exact else 'random'}"
            part = partial_call(g, n, nblk)
            OC.check_partial(tag, g, nblk, part, q)
            check_bits(tag + " rerun", partial_call(g, n, nblk), part)
            for mx in MAX_NORMS:
                total = finish_call(part, mx)
                OC.check_total(f"{tag} max_norm={mx}", part, mx, total, g, nblk, exact)
            check_bits(tag + " finish rerun", finish_call(part, MAX_NORMS[-1]), total)


@pytest.mark.parametrize("nblk", FINISH_NBLK)
def test_gradnorm_finish(nblk):
    part = input_storage(torch.rand(nblk, generator=torch.Generator(DEV).manual_seed(nblk), device=DEV) ** 4 * 100)
    for mx in MAX_NORMS + [3.0]:
        OC.check_total(f"finish nblk={nblk} max_norm={mx}", part, mx, finish_call(part, mx))
    ints = input_storage(torch.randint(0, 1000, (nblk,), generator=torch.Generator(DEV).manual_seed(nblk), device=DEV).float() * 0.25)
    total = finish_call(ints, 1.0)                               # integer partials: the sum is exact, the norm is one rounding of its root
    check_bits(f"finish nblk={nblk} exact", total[:1], ints.double().sum().sqrt().float().reshape(1))


@pytest.mark.parametrize("dtype", [BF, F32], ids=ids)
def test_gradnorm_of_zeros(dtype):
    g = input_storage(torch.zeros(1000, dtype=dtype, device=DEV))
    total = finish_call(partial_call(g, 1000, 4), 1.0)
    assert float(total[0]) == 0.0 and float(total[1]) == 1.0


def test_gradnorm_refusals():
    g = input_storage(torch.ones(64, dtype=BF, device=DEV))
    gp, gt = Guarded(4, F32, DEV), Guarded(2, F32, DEV)
    part, total = gp.view((4,), (1,)), gt.view((2,), (1,))
    assert rc("mm_gradnorm_partial", 0, p_(g), 64, p_(part), 0) == OC.ERR_ARG
    assert rc("mm_gradnorm_partial", 0, None, 64, p_(part), 4) == OC.ERR_ARG
    assert rc("mm_gradnorm_partial", 0, p_(g), 64, None, 4) == OC.ERR_ARG
    assert rc("mm_gradnorm_partial", 0, p_(g), -1, p_(part), 4) == OC.ERR_ARG
    assert rc("mm_gradnorm_partial", 0, p_(g) + 4, 32, p_(part), 4) == OC.ERR_ALIGN
    assert rc("mm_gradnorm_partial", 1, p_(g) + 4, 16, p_(part), 4) == OC.ERR_ALIGN
    ok = input_storage(torch.ones(4, device=DEV))
    assert rc("mm_gradnorm_finish", p_(ok), 0, f(1.0), p_(total)) == OC.ERR_ARG
    assert rc("mm_gradnorm_finish", None, 4, f(1.0), p_(total)) == OC.ERR_ARG
    assert rc("mm_gradnorm_finish", p_(ok), 4, f(1.0), None) == OC.ERR_ARG
    sync()
    for g_ in (gp, gt):
        assert bool((g_.buf.view(torch.int32) == SENTINEL[F32]).all()), "a refused call wrote to its output"


# ---- split / join ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SPLIT_N)
def test_master_split_join_on_constructed_bits(n):
    """Every low half x upper half (even, odd) x sign of optim_check.constructed_bits, and +-infinity.  NaN is left out: the
    conversion may quiet it, so its bits are not part of the contract."""
    w0, lossy0 = OC.constructed_bits(DEV)
    first = int(lossy0.nonzero()[0])                             # n = 1 gets a lossy element
    w, lossy = OC.tiled(w0.roll(-first), n), OC.tiled(lossy0.roll(-first), n)
    win = input_storage(w)
    gp = Guarded(n, BF, DEV)
    p = gp.view((n,), (1,))
    lo, glo = i16_storage(n)
    assert rc("mm_master_split", p_(win), n, p_(p), p_(lo)) == OC.OK
    sync()
    gp.verify("split p")
    glo.verify("split lo")                                      # no remainder of these values has the sentinel's pattern
    p_ref, lo_ref = OC.split_reference(w)
    check_bits("split p", p, p_ref)
    assert bool((lo == lo_ref).all()), "split lo"
    assert bool((lo[lossy] == 0x7FFF).all())
    gm = Guarded(n, F32, DEV)
    back = gm.view((n,), (1,))
    pin, loin = input_storage(p), input_storage(lo)
    assert rc("mm_master_join", p_(pin), p_(loin), n, p_(back)) == OC.OK
    sync()
    gm.verify("join")
    check_bits("join", back, OC.join_reference(p, lo))
    same = back.view(torch.int32) == w.view(torch.int32)
    assert bool((same == ~lossy).all()), "join(split(w)) == w exactly off the lossy set"
    check_bits("one ulp below on the lossy set", back[lossy], OC.ulp_below(w[lossy]))


def test_master_join_accepts_every_pair():
    """join is plain integer arithmetic: also the pairs no split produces (an odd p with lo = -0x8000)"""
    n = 4096
    gen = torch.Generator(DEV).manual_seed(1)
    p = (torch.randn(n, generator=gen, device=DEV) * 3).to(BF)
    lo = torch.randint(-32768, 32768, (n,), generator=gen, device=DEV).to(torch.int16)
    OC.plant_ties(p, lo, 0, 64)
    gm = Guarded(n, F32, DEV)
    back = gm.view((n,), (1,))
    pin, loin = input_storage(p), input_storage(lo)
    assert rc("mm_master_join", p_(pin), p_(loin), n, p_(back)) == OC.OK
    sync()
    gm.verify("join")
    check_bits("join", back, OC.join_reference(p, lo))


def test_master_split_join_refusals():
    w = input_storage(torch.ones(8, device=DEV))
    gp, gm = Guarded(8, BF, DEV), Guarded(8, F32, DEV)
    p, m = gp.view((8,), (1,)), gm.view((8,), (1,))
    lo, glo = i16_storage(8)
    assert rc("mm_master_split", p_(w), -1, p_(p), p_(lo)) == OC.ERR_ARG
    assert rc("mm_master_split", None, 8, p_(p), p_(lo)) == OC.ERR_ARG
    assert rc("mm_master_split", p_(w), 8, None, p_(lo)) == OC.ERR_ARG
    assert rc("mm_master_split", p_(w), 8, p_(p), None) == OC.ERR_ARG
    assert rc("mm_master_split", p_(w), 0, p_(p), p_(lo)) == OC.OK
    assert rc("mm_master_join", None, p_(lo), 8, p_(m)) == OC.ERR_ARG
    assert rc("mm_master_join", p_(p), None, 8, p_(m)) == OC.ERR_ARG
    assert rc("mm_master_join", p_(p), p_(lo), 8, None) == OC.ERR_ARG
    assert rc("mm_master_join", p_(p), p_(lo), -1, p_(m)) == OC.ERR_ARG
    assert rc("mm_master_join", p_(p), p_(lo), 0, p_(m)) == OC.OK
    sync()
    for g_ in (gp, gm, glo):
        assert bool((g_.buf.view(torch.int16 if g_.dtype == BF else torch.int32) == SENTINEL[g_.dtype]).all())
