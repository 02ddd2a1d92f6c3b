"""mm_sample on the GPU against the fp64 contract of tests/sampling_ref.py: the Philox draws bit for bit, kept sets and tokens,
draw statistics, determinism, and generate(do_sample=True, top_k / top_p / seed / generator) on the golden tiny models."""
import numpy as np
import pytest
import torch

from multimeditron_amd import kernels as K
from oracle import ref_cpu as R
from tests import sampling_ref as S
from tests.model_utils import build_from_golden

pytestmark = pytest.mark.gpu

CONFIGS = [(0, 1.0, 0.0), (1, 1.0, 0.0), (50, 1.0, 0.0), ("V", 1.0, 0.0), (0, 0.95, 0.0), (0, 1e-6, 0.0), (50, 0.9, 0.0),
           (0, 1.0, 0.05)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.mark.parametrize("rows", [1, 7, 1000])
@pytest.mark.parametrize("seed,offset", [(0, 0), (1, 5), (2**40 + 7, 2**33 + 1), (2**63 - 1, 123456789)])
def test_uniforms_match_python_philox(rows, seed, offset):
    u = K.sample_uniforms(seed, offset, rows).cpu().double().numpy()
    assert np.array_equal(u, S.uniforms(seed, offset, rows))


def _rows(kind, rows, V, rng):
    out = np.empty((rows, V), dtype=np.float32)
    for r in range(rows):
        x = rng.standard_normal(V).astype(np.float32) * 2.0
        spikes = rng.choice(V, size=min(V, 20), replace=False)
        x[spikes] += rng.exponential(6.0, size=spikes.shape[0]).astype(np.float32)       # heavy tail, like real logits
        if kind == "ties":                                                                  # plant ties at the 50th / 1st value
            order = np.argsort(-x, kind="stable")
            k = min(50, V) - 1
            x[order[max(0, k - 4): k + 5]] = x[order[k]]
            x[order[1]] = x[order[0]]
        elif kind == "ninf":
            x[rng.random(V) < 0.3] = -np.inf
            x[rng.integers(V)] = 1.0                                                        # at least one finite
        out[r] = x
    return out


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("V", [50, 1000, 128258])
@pytest.mark.parametrize("ragged", [False, True])
def test_kernel_matches_contract(dtype, V, ragged):
    rng = np.random.default_rng(V + 7 * ragged + (dtype == torch.bfloat16))
    ld = (V + 7) // 8 * 8 + (3 if ragged else 8)
    total = exact = 0
    for rows in (1, 4, 16):
        kinds = ["heavy", "ties", "ninf"]
        host = np.concatenate([_rows(kinds[i % 3], 1, V, rng) for i in range(rows)])
        buf = torch.zeros((rows, ld), dtype=dtype, device="cuda")
        buf[:, :V] = torch.from_numpy(host).to(dtype).cuda()
        lg = buf[:, :V]
        lg_host = lg.float().cpu().numpy()
        ws = K.sample_ws(rows, V, "cuda")
        for T in (0.1, 0.7, 1.5) if rows == 16 else (0.7,):
            for cfg in CONFIGS:
                k = V if cfg[0] == "V" else cfg[0]
                p, mp = np.float32(cfg[1]), np.float32(cfg[2])
                seed, offset = int(rng.integers(2**62)), int(rng.integers(1000))
                tok, th = K.sample(lg, V, T, top_k=k, top_p=float(p), min_p=float(mp), seed=seed, offset=offset, thresh=True, ws=ws)
                tok, th = tok.cpu().numpy(), th.cpu().numpy()
                ref = S.contract(lg_host, T, k, p, mp, seed=seed, offset=offset)
                for r in range(rows):
                    rr = ref[r]
                    total += 1
                    assert 0 <= tok[r] < V
                    assert rr["kept"][tok[r]] or rr["near_keep"], (T, cfg, r)
                    if p == 1.0 and mp == 0.0:
                        assert th[r] == rr["thresh"], (T, cfg, r, th[r], rr["thresh"])      # top-k: exact
                    elif not rr["near_keep"]:
                        assert th[r] == rr["thresh"], (T, cfg, r, th[r], rr["thresh"])
                    if tok[r] == rr["tok"] and th[r] == rr["thresh"]:
                        exact += 1
                    else:
                        assert rr["near_keep"] or rr["near_draw"], (T, cfg, r, tok[r], rr["tok"])
    assert exact >= 0.99 * total, (exact, total)


@pytest.mark.parametrize("cfg", [(0, 1.0), (8, 1.0), (0, 0.8)])
def test_draw_statistics(cfg):
    from scipy import stats
    V, N = 64, 65536
    rng = np.random.default_rng(3)
    row = (rng.standard_normal(V) * 1.5).astype(np.float32)
    lg = torch.from_numpy(np.tile(row, (N, 1))).cuda()
    tok = K.sample(lg, V, 1.0, top_k=cfg[0], top_p=cfg[1], seed=1234, offset=0).cpu().numpy()
    ref = S.contract_row(row, 1.0, cfg[0], np.float32(cfg[1]))
    kept = ref["kept"]
    assert kept[tok].all()                                            # nothing outside the kept set, ever
    w = np.exp(row.astype(np.float64) - row.max()) * kept
    p = w / w.sum()
    cnt = np.bincount(tok, minlength=V)[kept]
    chi = stats.chisquare(cnt, N * p[kept])
    assert chi.pvalue > 1e-4, chi


def test_determinism_and_offset():
    rng = np.random.default_rng(5)
    rows, V = 256, 1000
    lg = torch.from_numpy((rng.standard_normal((rows, V)) * 2).astype(np.float32)).cuda().to(torch.bfloat16)
    ws = K.sample_ws(rows, V, "cuda")
    a = K.sample(lg, V, 0.7, top_k=50, top_p=0.9, seed=99, offset=3, ws=ws).cpu()
    b = K.sample(lg, V, 0.7, top_k=50, top_p=0.9, seed=99, offset=3, ws=ws).cpu()
    c = K.sample(lg, V, 0.7, top_k=50, top_p=0.9, seed=99, offset=4, ws=ws).cpu()
    assert torch.equal(a, b)
    assert not torch.equal(a, c)


# ---------------------------------------------------------------------------------------------------------- generate()
MODELS = ["tiny_clip_llama", "tiny_clip_qwen2"]


@pytest.fixture(scope="module", params=MODELS)
def gold(request, golden_dir):
    return R.load_golden(request.param, golden_dir)


@pytest.fixture(scope="module")
def model_f32(gold, tmp_path_factory):
    meta, w, v = gold
    return build_from_golden(meta, w, tmp_path_factory.mktemp("s32"), "float32")


@pytest.mark.parametrize("case", ["left", "textonly"])
def test_generate_narrow_sampling_is_greedy(gold, model_f32, case):
    meta, w, v = gold
    batch = R.golden_batch(v, case)
    ids_k = model_f32.generate(batch, max_new_tokens=8, temperature=0.7, do_sample=True, top_k=1, seed=11)
    ids_p = model_f32.generate(batch, max_new_tokens=8, temperature=0.7, do_sample=True, top_p=1e-6, seed=12)
    assert torch.equal(ids_k, v[f"{case}.greedy_T0.7"])
    assert torch.equal(ids_p, v[f"{case}.greedy_T0.7"])


def test_generate_seed_and_generator_reproduce(gold, model_f32):
    meta, w, v = gold
    batch = R.golden_batch(v, "textonly")
    kw = dict(max_new_tokens=8, temperature=1.5, do_sample=True, top_p=0.99)
    a = model_f32.generate(batch, seed=2024, **kw)
    b = model_f32.generate(batch, seed=2024, **kw)
    assert torch.equal(a, b)
    g1, g2 = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    assert torch.equal(model_f32.generate(batch, generator=g1, **kw), model_f32.generate(batch, generator=g2, **kw))
    torch.manual_seed(31)
    c = model_f32.generate(batch, top_k=0, **kw)
    torch.manual_seed(31)
    d = model_f32.generate(batch, top_k=0, **kw)
    assert torch.equal(c, d)


@pytest.mark.parametrize("case", ["left", "textonly"])
def test_generate_matches_oracle_sampler(gold, model_f32, case):
    meta, w, v = gold
    batch = R.golden_batch(v, case)
    wf = {k: t.float() for k, t in w.items()}
    seed = 4242
    ids = model_f32.generate(batch, max_new_tokens=8, temperature=0.7, do_sample=True, top_p=0.9, seed=seed)
    ref, comp = S.sample_generate(wf, batch, meta, max_new_tokens=8, temperature=0.7, top_p=0.9, seed=seed, tol=2e-5)
    n = min(ids.shape[1], ref.shape[1])
    comp = comp[:, :n]
    assert torch.equal(ids[:, :n][comp], ref[:, :n][comp])
    assert int(comp.sum()) >= ids.shape[0] * 4, comp              # fp32 logits agree to ~1e-6: most steps compare


def test_generate_bf16_runs(gold, tmp_path_factory):
    meta, w, v = gold
    model = build_from_golden(meta, w, tmp_path_factory.mktemp("s16"), "bfloat16")
    batch = R.golden_batch(v, "left")
    V = meta["vocab_size"]
    for kw in (dict(top_k=1), dict(top_p=1e-6), dict(top_k=50, top_p=0.9, min_p=0.05), dict(seed=5)):
        ids = model.generate(batch, max_new_tokens=8, temperature=0.7, do_sample=True, **kw)
        assert ids.dtype == torch.int64 and ids.shape[0] == batch["input_ids"].shape[0] and 1 <= ids.shape[1] <= 8
        assert int(ids.min()) >= 0 and int(ids.max()) < V
