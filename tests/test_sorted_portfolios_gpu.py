"""The quantile-sort kernel (``csrc/k_qsort.hip``, ``Engine.sorted_portfolios``) on a real MI355X
against the numpy path of ``analysis.sorted_portfolios`` (the definition).

Panel A (12 x 150 x 46): masked stocks, an empty period, a period of 7 stocks (n < Q), a constant
column, a column of 4 distinct values and a column with both signed zeros. Panel B (3 x 2600 x 5):
long periods (a workgroup loops over 11 row chunks, buckets of 260 rows), one extra key that only
the lowest radix level separates (1 + k 2^-23) and one of random fp32 values of both signs.

Counts and breakpoints are exact. A bucket's fp64 sum differs from numpy's float64 sum over the
same rows only by the summation order: both are within (n - 1) 2^-53 sum|v| of the exact sum, so
their difference is within n 2^-52 sum|v|, plus one ulp of the result. Largest deviation seen:
profiles/sorted_portfolios_accuracy.txt."""
import numpy as np
import pytest
import torch

from deeplearninginassetpricing_paperreplication_amd.analysis import sorted_portfolios as sp
from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config
from deeplearninginassetpricing_paperreplication_amd.data.synthetic import generate_panel_fast
from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN

pytestmark = pytest.mark.gpu


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
    """batch, extra keys [E][T][N] (or None), extra values [K][T][N] (fp32 numpy)."""
    if name in _PANELS:
        return _PANELS[name]
    rng = np.random.default_rng(11)
    if name == "A":
        ret, feats, mask, mac = generate_panel_fast(12, 150, 46, 8, seed=0)
        assert bool(mask.all())
        mask = mask.clone()
        mask[:, torch.arange(150) % 7 == 3] = False      # masked stocks
        mask[5] = False                                  # an empty period
        assert int(mask.sum()) == 11 * 129
        keep = torch.nonzero(mask[2]).flatten()[::19][:7]
        mask[2] = False
        mask[2, keep] = True                             # n = 7 < Q
        assert int(mask[2].sum()) == 7
        feats = feats.clone()
        feats[:, :, 0] = 0.375                           # constant
        feats[:, :, 1] = torch.bucketize(feats[:, :, 1].contiguous(), torch.tensor([-0.5, 0.0, 0.5])).float() - 1.5   # 4 values
        z = torch.arange(150) % 5
        feats[:, z == 0, 2] = -0.0
        feats[:, z == 1, 2] = 0.0
        extra = None
    elif name == "B":
        ret, feats, mask, mac = generate_panel_fast(3, 2600, 5, 8, seed=1)
        assert bool(mask.all())
        perm = np.stack([rng.permutation(2600) for _ in range(3)])
        low = (1.0 + perm.astype(np.float64) * 2.0 ** -23).astype(np.float32)
        assert all(len(np.unique(low[t])) == 2600 for t in range(3))
        both = (rng.standard_normal((3, 2600)) * 10.0 ** rng.integers(-3, 4, (3, 2600))).astype(np.float32)
        extra = np.stack([low, both])
    else:                                                # wide layer-0 path: F + Dm > 128
        ret, feats, mask, mac = generate_panel_fast(4, 64, 130, 8, seed=2)
        mask = mask.clone()
        mask[1, ::3] = False
        extra = None
    T, N = mask.shape
    # extra values over 12 decades, so that the fp64 bucket sums do round
    vals = (rng.standard_normal((2, T, N)) * 10.0 ** rng.integers(-6, 7, (2, T, N))).astype(np.float32)
    mac = (mac - mac.mean(0)) / (mac.std(0, unbiased=False) + 1e-8)
    b = {"returns": ret, "individual_features": feats, "mask": mask, "macro_features": mac}
    _PANELS[name] = (b, extra, vals)
    return _PANELS[name]


def _spec(F):
    return AssetPricingGAN(default_cli_config(8, F, hidden_dim=[64, 64], rnn_dim=[4], dropout=0.05)).spec


def _run(name, precision, Q, G=1, cols=(), n_values=0, calls=1, use_extra=True):
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
    b, extra, vals = _panel(name)
    eng = GANEngine(_spec(b["individual_features"].shape[2]), G, max_epochs=4, precision=precision)
    eng.set_data(b)
    if name == "W":
        assert int(eng.desc["wide"]) == 1
    ek = torch.as_tensor(extra).cuda().contiguous() if extra is not None and use_extra else None
    vv = torch.as_tensor(vals[:n_values]).cuda().contiguous() if n_values else None
    torch.cuda.synchronize()
    out = [eng.eng.sorted_portfolios(0, Q, list(cols), ek.data_ptr() if ek is not None else 0,
                                     0 if ek is None else ek.shape[0], vv.data_ptr() if vv is not None else 0, n_values)
           for _ in range(calls)]
    eng.eng.sync()
    return out[0] if calls == 1 else out


_REFS = {}


def _ref(name, precision, Q, n_values=0):
    """The numpy path on the keys the engine holds, and the same with |values| (for the bound)."""
    key = (name, precision, Q, n_values)
    if key not in _REFS:
        b, extra, vals = _panel(name)
        f = b["individual_features"]
        keys = (_bf16_round(f) if precision == "bf16" else f).numpy().astype(np.float32)
        if extra is not None:
            keys = np.concatenate([keys, np.moveaxis(extra, 0, 2)], axis=2)
        v = np.concatenate([b["returns"].numpy().astype(np.float32)[:, :, None],
                            np.moveaxis(vals[:n_values], 0, 2)], axis=2)
        m = b["mask"].numpy()
        _REFS[key] = (sp.sort_buckets_numpy(keys, m, v, Q), sp.sort_buckets_numpy(keys, m, np.abs(v), Q)["sum"])
    return _REFS[key]


def _check(got, ref, absum, mask, sel=None):
    """Exact counts and breakpoints, sums within the fp64 accumulation bound; returns the largest
    deviation as a share of the bound."""
    rc, rs, rb = ref["count"], ref["sum"], ref["breaks"]
    if sel is not None:
        rc, rs, rb, absum = rc[:, sel], rs[:, sel], rb[:, sel], absum[:, sel]
    cnt, sm, br = np.asarray(got["count"]), np.asarray(got["sum"]), np.asarray(got["breaks"])
    assert cnt.dtype == np.int32 and sm.dtype == np.float64 and br.dtype == np.float32
    np.testing.assert_array_equal(cnt, rc)
    np.testing.assert_array_equal(br.view(np.uint32), rb.astype(np.float32).view(np.uint32))
    nt = mask.sum(1).astype(np.float64)
    assert (cnt.sum(-1) == nt[:, None]).all()
    assert int(got["rows"]) == int(mask.sum())
    bound = nt[:, None, None, None] * 2.0 ** -52 * absum + np.spacing(np.abs(rs))
    dev = np.abs(sm - rs)
    worst = float((dev / bound).max())
    print(f"largest |sum - numpy| / bound = {worst:.3f}, largest |sum - numpy| = {dev.max():.3e}")
    assert (dev <= bound).all()
    return worst


@pytest.mark.parametrize("Q", [10, 5, 16])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_panel_a_matches_numpy(precision, Q):
    b = _panel("A")[0]
    mask = b["mask"].numpy()
    got = _run("A", precision, Q)
    ref, absum = _ref("A", precision, Q)
    _check(got, ref, absum, mask)
    cnt, br = np.asarray(got["count"]), np.asarray(got["breaks"])
    assert (cnt[5] == 0).all() and np.isnan(br[5]).all() and (np.asarray(got["sum"])[5] == 0).all()
    assert (cnt[:, 0, 0] == mask.sum(1)).all()           # the constant column: everything in bucket 0
    assert ((cnt[2] > 0).sum(-1) <= 7).all()             # n = 7 < Q leaves buckets empty
    assert float(got["gpu_ms"]) > 0


@pytest.mark.parametrize("Q", [10, 5, 16])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_panel_b_long_periods_and_extra_keys(precision, Q):
    mask = _panel("B")[0]["mask"].numpy()
    got = _run("B", precision, Q, n_values=2)             # (the extra values are summed too)
    ref, absum = _ref("B", precision, Q, n_values=2)
    _check(got, ref, absum, mask)
    cnt = np.asarray(got["count"])
    assert np.asarray(got["sum"]).shape == (3, 7, Q, 3)
    # tie-free fp32 keys: every bucket holds floor or ceil of n / Q rows (260 for Q = 10)
    assert cnt[:, 5:].min() >= 2600 // Q and cnt[:, 5:].max() <= -(-2600 // Q)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_repeatable_and_independent_of_the_models(precision):
    a, b2 = _run("A", precision, 10, n_values=2, calls=2)
    assert np.asarray(a["sum"]).tobytes() == np.asarray(b2["sum"]).tobytes()
    c = _run("A", precision, 10, G=3, n_values=2)
    for k in ("count", "sum", "breaks"):
        assert np.asarray(a[k]).tobytes() == np.asarray(c[k]).tobytes()
    ref, absum = _ref("A", precision, 10, n_values=2)
    _check(a, ref, absum, _panel("A")[0]["mask"].numpy())


def test_column_subset_equals_slices():
    full = _run("A", "bf16", 10)
    sub = _run("A", "bf16", 10, cols=[3, 0, 45])
    for k in ("count", "sum", "breaks"):
        assert np.asarray(sub[k]).tobytes() == np.ascontiguousarray(np.asarray(full[k])[:, [3, 0, 45]]).tobytes()
    ref, absum = _ref("A", "bf16", 10)
    _check(sub, ref, absum, _panel("A")[0]["mask"].numpy(), sel=[3, 0, 45])


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_wide_path_engine(precision):
    mask = _panel("W")[0]["mask"].numpy()
    got = _run("W", precision, 10, n_values=1)
    ref, absum = _ref("W", precision, 10, n_values=1)
    _check(got, ref, absum, mask)
    assert np.asarray(got["count"]).shape == (4, 130, 10)


def test_bad_arguments():
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
    b, _, vals = _panel("A")
    eng = GANEngine(_spec(46), 1, max_epochs=4)
    eng.set_data(b)
    vv = torch.zeros(5, 12, 150, device="cuda")
    torch.cuda.synchronize()
    e = eng.eng
    for kw in (dict(quantiles=1), dict(quantiles=17), dict(cols=[46]), dict(cols=[-1]),
               dict(values=vv.data_ptr(), n_values=5), dict(s=3)):
        with pytest.raises(ValueError):
            e.sorted_portfolios(**{"s": 0, **kw})
    with pytest.raises(RuntimeError):
        e.sorted_portfolios(1)                           # split not set
    ok = e.sorted_portfolios(0, quantiles=2, cols=[45])
    assert np.asarray(ok["count"]).shape == (12, 1, 2)


def test_python_api_cuda_matches_cpu():
    """One ensemble weight handed to both devices (evaluated by the engine): counts are equal once
    the CPU path sorts the bf16-rounded characteristics, and the priced results agree to 1e-9.
    With each device evaluating the models itself the weights differ by the towers' precision, so
    only what does not depend on them is compared: the counts and the characteristic-sorted
    returns."""
    b = _panel("A")[0]
    models = []
    cfg = default_cli_config(8, 46, hidden_dim=[64, 64], rnn_dim=[4], dropout=0.05)
    for g in range(2):
        torch.manual_seed(100 + g)
        models.append(AssetPricingGAN(cfg).eval())
    w = sp._gpu_weights(models, b).cpu().numpy()
    br = dict(b)
    br["individual_features"] = _bf16_round(b["individual_features"])
    gpu = sp.sorted_portfolios(models, b, device="cuda", weights=w)
    cpu = sp.sorted_portfolios(models, br, device="cpu", weights=w)
    assert gpu["names"] == cpu["names"] and len(gpu["names"]) == 47
    np.testing.assert_array_equal(gpu["count"], cpu["count"])
    r, m = b["returns"].numpy(), b["mask"].numpy()
    pg, pc = sp.price_portfolios(gpu, w, r, m), sp.price_portfolios(cpu, w, r, m)
    for k in ("mean_ret", "alpha", "t_alpha", "ev_asset", "hml", "hml_sharpe", "ev", "xs_r2", "mean_abs_alpha"):
        np.testing.assert_allclose(np.asarray(pg[k]), np.asarray(pc[k]), rtol=1e-9, atol=0, equal_nan=True, err_msg=k)
    own_g = sp.sorted_portfolios(models, b, device="cuda")
    own_c = sp.sorted_portfolios(models, br, device="cpu")
    np.testing.assert_array_equal(own_g["count"][:, :46], own_c["count"][:, :46])
    np.testing.assert_array_equal(own_g["count"].sum(-1), own_c["count"].sum(-1))
    np.testing.assert_allclose(own_g["returns"][:, :46], own_c["returns"][:, :46], rtol=1e-9, atol=1e-15, equal_nan=True)
    assert np.isfinite(own_g["loading"][own_g["count"] > 0]).all()


def test_evaluate_ensemble_end_to_end(shipped_data, capsys):
    """``--sorted_portfolios`` on both devices: the same report layout and assets, the rest of the
    result unchanged. (The numbers differ by the towers' precision and by the 0.4 % of rows the
    bf16 panel moves across a breakpoint, so only the structure is compared.)"""
    import os
    import golden_cases as gc
    from deeplearninginassetpricing_paperreplication_amd.analysis import ensemble as ens
    ckpts = [gc.path(os.path.join("ensemble_ckpt", f"m{seed}")) for seed in (1, 2)]
    plain = ens.evaluate_ensemble(ckpts, shipped_data, device="cuda", verbose=False)
    capsys.readouterr()
    gpu = ens.evaluate_ensemble(ckpts, shipped_data, device="cuda", verbose=True, sorted_portfolios=True)
    tg = capsys.readouterr().out
    cpu = ens.evaluate_ensemble(ckpts, shipped_data, device="cpu", verbose=True, sorted_portfolios=True)
    tc = capsys.readouterr().out
    print(tg[tg.index("SORTED PORTFOLIOS"):])
    print(tc[tc.index("SORTED PORTFOLIOS"):])
    for k in plain:
        assert gpu[k] == plain[k]
    g, c = gpu["sorted_portfolios"], cpu["sorted_portfolios"]
    assert "gpu_ms" in g["portfolios"] and "gpu_ms" not in c["portfolios"]
    assert g["portfolios"]["names"] == c["portfolios"]["names"] and len(g["portfolios"]["names"]) == 47
    assert g["portfolios"]["count"].shape == c["portfolios"]["count"].shape == (60, 47, 10)
    np.testing.assert_array_equal(g["portfolios"]["count"].sum(-1), c["portfolios"]["count"].sum(-1))
    assert g["priced"]["assets"] == c["priced"]["assets"] == 470
    assert np.isfinite(g["priced"]["hml"]).all() and np.isfinite(g["priced"]["ev"])
    assert len(tg[tg.index("SORTED PORTFOLIOS"):].splitlines()) == len(tc[tc.index("SORTED PORTFOLIOS"):].splitlines())
