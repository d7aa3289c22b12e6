"""The linear-benchmark kernels (``csrc/k_linport.hip``: ``Engine.managed_portfolios``,
``Engine.linear_portfolios``) on a real MI355X against the numpy path of ``analysis.benchmarks`` on
the features as stored (bf16-rounded for the bf16 panel).

Panel A (12 x 150 x 46): masked stocks, an empty period, a period of 7 stocks (less than one
16-row tile), a constant column and columns scaled over six decades. Panel B (3 x 2600 x 5):
six segments per period (5 x 512 + 40 rows, a ragged last tile of 8 rows; one period ends on a
whole tile, one on a tile with a single row), F = 5 is no multiple of the MFMA k = 4. Panel W (4 x 64 x 130): the wide layer-0 path.

Bounds (u = 2^-24, Fp = F rounded up to 4). ``n`` is exact. A managed sum differs from numpy's
float64 sum by the summation order only: within n 2^-52 sum|x R| plus one ulp. The kernel forms
w = x . theta in fp32 (exact products of the stored fp32 / bf16 values, at most Fp roundings in the
accumulation; the padded k-steps add exact zeros) and v = fp32(w - c): a row's v is within
d_i = (Fp + 2) u (sum_f |x th| + |c|) of the float64 value. So S1 and SA are within sum d_i, SR
within sum d_i |R_i| and S2 within sum (2 |v| d_i + d_i^2), each plus n 2^-52 times the absolute
sum of its terms and one ulp of the result. Only the fp32-input MFMA path exists (no bf16 split of
theta), in both panel precisions. Largest ratios seen: profiles/linear_benchmarks_accuracy.txt."""
import numpy as np
import pytest
import torch

from deeplearninginassetpricing_paperreplication_amd.analysis import benchmarks as bm
from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config
from deeplearninginassetpricing_paperreplication_amd.data.synthetic import generate_panel_fast
from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = 12345.0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeplearninginassetpricing_paperreplication_amd.ops import native
    native.load(required=True)


def _bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


_PANELS = {}


def _panel(name):
    if name in _PANELS:
        return _PANELS[name]
    if name == "A":
        ret, feats, mask, mac = generate_panel_fast(12, 150, 46, 8, seed=0)
        assert bool(mask.all())
        mask = mask.clone()
        mask[:, torch.arange(150) % 7 == 3] = False      # masked stocks
        mask[5] = False                                  # an empty period
        keep = torch.nonzero(mask[2]).flatten()[::19][:7]
        mask[2] = False
        mask[2, keep] = True                             # 7 stocks: less than one 16-row tile
        assert int(mask[2].sum()) == 7
        feats = feats.clone()
        feats[:, :, 0] = 0.375                           # constant
        feats[:, :, 40:46] *= torch.tensor([1e-3, 1e-2, 1e-1, 10.0, 100.0, 1e3])   # several decades
    elif name == "B":
        ret, feats, mask, mac = generate_panel_fast(3, 2600, 5, 8, seed=1)
        assert bool(mask.all())
        mask = mask.clone()
        mask[1, :24] = False                             # 2576 rows: whole tiles only
        mask[2, :23] = False                             # 2577 rows: a last tile with a single row
    elif name == "W":                                    # wide layer-0 path: F + Dm > 128
        ret, feats, mask, mac = generate_panel_fast(4, 64, 130, 8, seed=2)
        mask = mask.clone()
        mask[1, ::3] = False
    else:                                                # "E": a split without a valid row
        ret, feats, mask, mac = generate_panel_fast(3, 20, 5, 8, seed=3)
        mask = torch.zeros_like(mask)
    mac = (mac - mac.mean(0)) / (mac.std(0, unbiased=False) + 1e-8)
    _PANELS[name] = {"returns": ret, "individual_features": feats, "mask": mask, "macro_features": mac}
    return _PANELS[name]


def _np(name, precision):
    """(x as stored [T][N][F] fp32, returns, mask) in numpy."""
    b = _panel(name)
    f = b["individual_features"]
    x = (_bf16_round(f) if precision == "bf16" else f).numpy().astype(np.float32)
    return x, b["returns"].numpy().astype(np.float32), b["mask"].numpy()


def _spec(F):
    return AssetPricingGAN(default_cli_config(8, F, hidden_dim=[64, 64], rnn_dim=[4], dropout=0.05)).spec


def _engine(name, precision):
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
    b = _panel(name)
    eng = GANEngine(_spec(b["individual_features"].shape[2]), 1, max_epochs=4, precision=precision)
    eng.set_data(b)
    assert int(eng.desc["wide"]) == (1 if name == "W" else 0)
    return eng


def _theta(K, F, seed=7):
    """Both signs, magnitudes over three decades."""
    rng = np.random.default_rng(seed + 100 * K + F)
    return (rng.standard_normal((K, F)) * 10.0 ** rng.uniform(-1.5, 1.5, (K, F))).astype(np.float32)


def _linport(eng, th, c=None, weights=False):
    """Engine.linear_portfolios; with ``weights`` also the sentinel-filled dense buffer."""
    T, N = (int(v) for v in (eng.splits[0].T, eng.splits[0].N))
    w = torch.full((th.shape[0], T, N), SENTINEL, dtype=torch.float32, device="cuda") if weights else None
    torch.cuda.synchronize()
    r = eng.eng.linear_portfolios(0, th, c, w.data_ptr() if weights else 0)
    eng.eng.sync()
    return (r, w.cpu().numpy()) if weights else r


def _managed_bound(x, r, m):
    n = m.sum(1).astype(np.float64)[:, None]
    ax = np.abs(x.astype(np.float64)) * m[:, :, None]
    return n * 2.0 ** -52 * ax.sum(1), n * 2.0 ** -52 * (ax * np.abs(r.astype(np.float64))[:, :, None]).sum(1)


def _check_managed(got, x, r, m):
    ref = bm.managed_portfolios_numpy(x, r, m)
    bx, bxr = _managed_bound(x, r, m)
    assert np.asarray(got["n"]).dtype == np.int32
    np.testing.assert_array_equal(np.asarray(got["n"]), ref["n"])
    assert int(got["rows"]) == ref["rows"]
    worst = 0.0
    for k, b in (("sum_x", bx), ("sum_xr", bxr)):
        g = np.asarray(got[k])
        assert g.dtype == np.float64 and g.shape == ref[k].shape
        bound = b + np.spacing(np.abs(ref[k]))
        dev = np.abs(g - ref[k])
        worst = max(worst, float((dev / bound).max()))
        assert (dev <= bound).all(), k
    print(f"managed: largest |sum - numpy| / bound = {worst:.3f}")
    return ref


_ORACLE = {}


def _oracle(name, precision, K, centered):
    """numpy sums, the centre used, and the bounds of the module docstring, per (t, k)."""
    key = (name, precision, K, centered)
    if key in _ORACLE:
        return _ORACLE[key]
    x, r, m = _np(name, precision)
    T, N, F = x.shape
    th = _theta(K, F)
    c = bm.center_from_managed(bm.managed_portfolios_numpy(x, r, m), th, "mean") if centered else None
    ref = bm.linear_sums_numpy(x, r, m, th, c)
    Fp = (F + 3) // 4 * 4
    cc = np.zeros((T, K)) if c is None else c.astype(np.float64)
    bound = {k: np.zeros((T, K)) for k in ("s1", "sa", "s2", "sr")}
    ath, th64 = np.abs(th).astype(np.float64), th.astype(np.float64)
    for t in range(T):
        idx = np.nonzero(m[t])[0]
        if not idx.size:
            continue
        xt = x[t, idx].astype(np.float64)
        rt = np.abs(r[t, idx].astype(np.float64))[:, None]
        v = np.abs(xt @ th64.T - cc[t][None])
        d = (Fp + 2) * U * (np.abs(xt) @ ath.T + np.abs(cc[t])[None])
        s = idx.size * 2.0 ** -52
        bound["s1"][t] = d.sum(0) + s * (v + np.abs(cc[t])[None] + d).sum(0)
        bound["sa"][t] = d.sum(0) + s * (v + d).sum(0)
        bound["sr"][t] = (d * rt).sum(0) + s * ((v + d) * rt).sum(0)
        bound["s2"][t] = (2 * v * d + d * d).sum(0) + s * ((v + d) ** 2).sum(0)
    for k in bound:
        bound[k] += np.spacing(np.abs(ref[k]))
    _ORACLE[key] = (th, c, ref, bound)
    return _ORACLE[key]


def _check_sums(got, ref, bound, tag=""):
    np.testing.assert_array_equal(np.asarray(got["n"]), ref["n"])
    assert int(got["rows"]) == ref["rows"]
    n = ref["n"].astype(np.float64)
    for k, a in (("sum_r", np.abs(ref["sum_r"])), ("sum_rr", ref["sum_rr"])):
        # (bounded by the absolute sum: sum |R| >= |sum R|, so use sum_rr's own value and sqrt(n sum_rr))
        lim = n * 2.0 ** -52 * (np.sqrt(n * ref["sum_rr"]) if k == "sum_r" else ref["sum_rr"]) + np.spacing(a)
        assert (np.abs(np.asarray(got[k]) - ref[k]) <= lim).all(), k
    worst = {}
    for k in ("s1", "sa", "s2", "sr"):
        g = np.asarray(got[k])
        assert g.dtype == np.float64 and g.shape == ref[k].shape
        dev = np.abs(g - ref[k])
        worst[k] = float((dev / bound[k]).max())
        assert (dev <= bound[k]).all(), (k, worst[k])
    print(f"linport {tag}: largest deviation / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return worst


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["A", "B", "W"])
def test_managed_matches_numpy(name, precision):
    eng = _engine(name, precision)
    x, r, m = _np(name, precision)
    got = eng.eng.managed_portfolios(0)
    _check_managed(got, x, r, m)
    again = eng.eng.managed_portfolios(0)
    for k in ("sum_x", "sum_xr", "n"):
        assert np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes()
    if name == "A":
        assert (np.asarray(got["sum_x"])[5] == 0).all() and np.asarray(got["n"])[5] == 0
        np.testing.assert_array_equal(np.asarray(got["sum_x"])[:, 0], 0.375 * m.sum(1))   # the constant column, exact
    assert float(got["gpu_ms"]) > 0


@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("K", [1, 17, 64])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_linport_matches_numpy(name, precision, K, centered):
    eng = _engine(name, precision)
    th, c, ref, bound = _oracle(name, precision, K, centered)
    got = _linport(eng, th, c)
    _check_sums(got, ref, bound, f"{name} {precision} K={K} center={centered}")
    if name == "A":
        for k in ("s1", "sa", "s2", "sr"):
            assert (np.asarray(got[k])[5] == 0).all()                # the empty period
    assert float(got["gpu_ms"]) > 0


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_wide_path(precision):
    eng = _engine("W", precision)
    th, c, ref, bound = _oracle("W", precision, 17, True)
    if eng.eng.linear_supported():
        _check_sums(_linport(eng, th, c), ref, bound, f"W {precision}")
    else:
        with pytest.raises(ValueError):
            eng.eng.linear_portfolios(0, th, c, 0)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_identity_theta_equals_managed(name, precision):
    eng = _engine(name, precision)
    x, r, m = _np(name, precision)
    F = x.shape[2]
    man = eng.eng.managed_portfolios(0)
    got = _linport(eng, np.eye(F, dtype=np.float32))
    bx, bxr = _managed_bound(x, r, m)
    for k, ref, b in (("s1", np.asarray(man["sum_x"]), bx), ("sr", np.asarray(man["sum_xr"]), bxr)):
        assert (np.abs(np.asarray(got[k]) - ref) <= b + np.spacing(np.abs(ref))).all(), k


@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_written_weights_are_the_summed_numbers(name, precision, centered):
    """``w_out`` keeps the sentinel at every invalid (t, i); its valid entries, summed in float64,
    reproduce S1 - n c, SA, S2 and SR up to the summation order."""
    eng = _engine(name, precision)
    th, c, ref, bound = _oracle(name, precision, 17, centered)
    got, w = _linport(eng, th, c, weights=True)
    x, r, m = _np(name, precision)
    assert (w[:, ~m] == SENTINEL).all()
    v = np.where(m[None], w, 0.0).astype(np.float64)               # [K][T][N]
    assert np.isfinite(v).all()
    rr = np.where(m, r, 0).astype(np.float64)
    n = m.sum(1).astype(np.float64)[None, :]
    cc = np.zeros_like(ref["s1"]) if c is None else c.astype(np.float64)
    s = n * 2.0 ** -52
    av = np.abs(v).sum(2)
    sums = {"s1": (v.sum(2) + n * cc.T, av + n * np.abs(cc.T)), "sa": (av, av), "s2": ((v * v).sum(2), (v * v).sum(2)),
            "sr": ((v * rr[None]).sum(2), (np.abs(v) * np.abs(rr)[None]).sum(2))}
    for k, (val, absum) in sums.items():
        g = np.asarray(got[k]).T
        assert (np.abs(g - val) <= s * absum + np.spacing(np.abs(val))).all(), k
    plain = _linport(eng, th, c)                                    # the sums do not depend on w_out
    for k in ("s1", "sa", "s2", "sr"):
        assert np.asarray(plain[k]).tobytes() == np.asarray(got[k]).tobytes()
    _check_sums(got, ref, bound, f"{name} {precision} w_out")


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_repeatable_and_pad_columns_ignored(precision):
    """Two calls are bitwise equal, and so is a split whose stored rows carry NaN in every column
    >= F. ``set_split_dense`` zero-fills those columns, so the poisoned rows go in through
    ``Engine.set_split`` (host-compacted rows)."""
    from deeplearninginassetpricing_paperreplication_amd.engine.panel import prepare_split
    eng = _engine("A", precision)
    th, c, ref, bound = _oracle("A", precision, 64, True)
    a, b2 = _linport(eng, th, c), _linport(eng, th, c)
    keys = ("s1", "sa", "s2", "sr", "sum_r", "sum_rr", "n")
    for k in keys:
        assert np.asarray(a[k]).tobytes() == np.asarray(b2[k]).tobytes()
    man = eng.eng.managed_portfolios(0)
    KP, F = eng.KP, 46
    assert KP > F
    ps = prepare_split(_panel("A"), KP, fp32=precision == "fp32")
    X = ps.X.copy()
    if precision == "fp32":
        X.view(np.float32).reshape(ps.R, KP)[:, F:] = np.nan
    else:
        X.reshape(ps.R, KP)[:, F:] = 0x7FC0
    eng.eng.set_split(0, X, ps.rowti, ps.row_ptr, ps.Rm, ps.mask, ps.macro.reshape(-1), int(ps.T), int(ps.N))
    p = _linport(eng, th, c)
    for k in keys:
        assert np.isfinite(np.asarray(p[k])).all()
        assert np.asarray(p[k]).tobytes() == np.asarray(a[k]).tobytes()
    pm = eng.eng.managed_portfolios(0)
    for k in ("sum_x", "sum_xr", "n"):
        assert np.asarray(pm[k]).tobytes() == np.asarray(man[k]).tobytes()


def test_empty_split_and_bad_arguments():
    eng = _engine("E", "bf16")
    th = _theta(3, 5)
    r = eng.eng.linear_portfolios(0, th, None, 0)
    for k in ("s1", "sa", "s2", "sr"):
        assert np.asarray(r[k]).shape == (3, 3) and (np.asarray(r[k]) == 0).all()
    assert (np.asarray(r["n"]) == 0).all() and int(r["rows"]) == 0 and float(r["gpu_ms"]) == 0
    mp = eng.eng.managed_portfolios(0)
    assert np.asarray(mp["sum_x"]).shape == (3, 5) and (np.asarray(mp["sum_xr"]) == 0).all() and float(mp["gpu_ms"]) == 0
    e = _engine("A", "bf16").eng
    assert e.linear_supported() is True
    ok = _theta(2, 46)
    for args in ((0, np.zeros((0, 46), np.float32), None, 0), (0, _theta(65, 46), None, 0), (0, _theta(2, 45), None, 0),
                 (0, ok[0], None, 0), (0, ok, np.zeros((12, 3), np.float32), 0), (0, ok, np.zeros((11, 2), np.float32), 0),
                 (3, ok, None, 0)):
        with pytest.raises(ValueError):
            e.linear_portfolios(*args)
    with pytest.raises(ValueError):
        e.managed_portfolios(-1)
    with pytest.raises(RuntimeError):
        e.linear_portfolios(1, ok, None, 0)                          # split not set
    with pytest.raises(RuntimeError):
        e.managed_portfolios(2)
    assert np.asarray(e.linear_portfolios(0, ok, np.zeros((12, 2), np.float32), 0)["s1"]).shape == (12, 2)


def test_python_api_cuda_matches_cpu():
    """``linear_benchmarks`` on both devices with the same candidates, fp32 panel: per-candidate
    factors within the bounds (F = SR / SA: |dF| <= (b_SR + |F| b_SA) / (SA - b_SA), plus the centre's
    own difference, which the d_i already allow for), and a stable selection: the candidate the
    GPU chooses has a CPU Sharpe no lower than the CPU's best minus 2 max_k |sharpe_gpu - sharpe_cpu|."""
    b = _panel("A")
    rng = np.random.default_rng(21)
    tt = rng.permutation(12)
    batches = {}
    for name, sel in (("train", tt[:6]), ("valid", tt[6:9]), ("test", tt[9:])):
        sel = np.sort(sel)
        batches[name] = {k: v[sel].contiguous() for k, v in b.items()}
    th = _theta(9, 46, seed=3)
    cpu = bm.linear_benchmarks(batches, device="cpu", thetas=th)
    gpu = bm.linear_benchmarks(batches, device="cuda", thetas=th, precision="fp32")
    assert gpu["device"] == "cuda" and cpu["device"] == "cpu" and "gpu_ms" in gpu
    worst = 0.0
    for s in bm.SPLITS:
        x, r, m = (batches[s][k].numpy() for k in ("individual_features", "returns", "mask"))
        T, N, F = x.shape
        Fp = (F + 3) // 4 * 4
        c = bm.center_from_managed(bm.managed_portfolios_numpy(x, r, m), th)
        ref = bm.linear_sums_numpy(x, r, m, th, c)
        bsa, bsr = np.zeros_like(ref["sa"]), np.zeros_like(ref["sr"])
        for t in range(T):
            idx = np.nonzero(m[t])[0]
            if idx.size:
                d = (Fp + 2) * U * (np.abs(x[t, idx].astype(np.float64)) @ np.abs(th).astype(np.float64).T
                                    + 2 * np.abs(c[t].astype(np.float64))[None])
                bsa[t], bsr[t] = d.sum(0), (d * np.abs(r[t, idx].astype(np.float64))[:, None]).sum(0)
        fc, fg = cpu["candidates"][s]["factor"], gpu["candidates"][s]["factor"]
        ok = ref["sa"] > 1e-8
        lim = np.where(ok, (bsr + np.abs(fc) * bsa) / np.where(ok, ref["sa"] - bsa, 1.0), bsr) * (1 + 1e-9) + 1e-300
        assert (ref["sa"][ok] > 2 * bsa[ok]).all()
        dev = np.abs(fg - fc)
        worst = max(worst, float((dev / lim).max()))
        assert (dev <= lim).all(), s
    print(f"factors: largest |gpu - cpu| / bound = {worst:.3f}")
    sc, sg = cpu["candidates"]["valid"]["sharpe"], gpu["candidates"]["valid"]["sharpe"]
    assert sc[gpu["EN"]["index"]] >= sc.max() - 2 * np.abs(sg - sc).max()
    for s in bm.SPLITS:
        m = batches[s]["mask"].numpy()
        wg, wc = gpu["EN"]["weights"][s], cpu["EN"]["weights"][s]
        assert wg.shape == wc.shape and (wg[~m] == 0).all()
        assert np.allclose(np.abs(wg).sum(1)[m.any(1)], 1.0, atol=1e-6)     # L1-normalised (fp32 v, float64 SA)
