"""The double-sort kernel (``csrc/k_qsort2.hip``, ``Engine.double_sorted_portfolios``) on a real
MI355X against the numpy path of ``analysis.sorted_portfolios`` (``double_sort_numpy``, the
definition), on the keys the engine holds (bf16-rounded characteristics for a bf16 panel).

Panel A (12 x 150 x 46): masked stocks, an empty period (5), a period of 7 stocks (2: with
Qa = 5 every first-key bucket has 1 or 2 rows, fewer than Qb), a constant column (0: as first key
every row is in bucket 0 and the other buckets are empty, their breakpoints NaN), a column of 4
distinct values (1) and a column with both signed zeros (2). Panel B (3 x 2600 x 5): long periods
(a workgroup loops over 11 row chunks), one extra key that only the lowest radix level separates
(1 + k 2^-23) and one of random fp32 values of both signs; its pairs mix a bf16 characteristic
with an fp32 extra key in either order (different key widths). Panel W (4 x 64 x 130): the wide
layer-0 path.

Counts and both breakpoint arrays are exact. A cell's fp64 sum differs from numpy's float64 sum
over the same rows only by the summation order: both are within (m - 1) 2^-53 sum|v| of the exact
sum for a cell of m <= n rows, so their difference is within n 2^-52 sum|v|, plus one ulp of the
result (the bound of the single-sort test, per cell). Largest deviation seen:
profiles/double_sorts_accuracy.txt."""
import numpy as np
import pytest
import torch

from deeplearninginassetpricing_paperreplication_amd.analysis import sorted_portfolios as sp
from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config
from deeplearninginassetpricing_paperreplication_amd.data.synthetic import generate_panel_fast
from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN

pytestmark = pytest.mark.gpu

PAIRS_A = [(0, 3), (1, 2), (3, 1), (4, 4), (7, 45)]
PAIRS_B = [(1, 5), (5, 2), (6, 3), (5, 6), (6, 5), (6, 6)]     # 5, 6: the extra keys
SHAPES = [(5, 5), (2, 3), (6, 6), (3, 12)]


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
        mask[2, keep] = True                             # n = 7
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
        assert all(len(np.unique(both[t])) == 2600 for t in range(3))
        extra = np.stack([low, both])
    else:                                                # wide layer-0 path: F + Dm > 128
        ret, feats, mask, mac = generate_panel_fast(4, 64, 130, 8, seed=2)
        mask = mask.clone()
        mask[1, ::3] = False
        extra = None
    T, N = mask.shape
    # extra values over 12 decades, so that the fp64 cell sums do round
    vals = (rng.standard_normal((2, T, N)) * 10.0 ** rng.integers(-6, 7, (2, T, N))).astype(np.float32)
    mac = (mac - mac.mean(0)) / (mac.std(0, unbiased=False) + 1e-8)
    b = {"returns": ret, "individual_features": feats, "mask": mask, "macro_features": mac}
    _PANELS[name] = (b, extra, vals)
    return _PANELS[name]


def _spec(F):
    return AssetPricingGAN(default_cli_config(8, F, hidden_dim=[64, 64], rnn_dim=[4], dropout=0.05)).spec


_ENGINES = {}


def _engine(name, precision, G=1):
    """One engine per (panel, precision, model count), with the panel's extra arrays on the device."""
    key = (name, precision, G)
    if key not in _ENGINES:
        from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
        b, extra, vals = _panel(name)
        eng = GANEngine(_spec(b["individual_features"].shape[2]), G, max_epochs=4, precision=precision)
        eng.set_data(b)
        if name == "W":
            assert int(eng.desc["wide"]) == 1
        ek = torch.as_tensor(extra).cuda().contiguous() if extra is not None else None
        vv = torch.as_tensor(vals).cuda().contiguous()
        torch.cuda.synchronize()
        _ENGINES[key] = (eng, ek, vv)
    return _ENGINES[key]


def _run(name, precision, pairs, Q, conditional=True, G=1, n_values=0):
    eng, ek, vv = _engine(name, precision, G)
    out = eng.eng.double_sorted_portfolios(0, list(pairs), Q[0], Q[1], conditional, ek.data_ptr() if ek is not None else 0,
                                           0 if ek is None else ek.shape[0], vv.data_ptr() if n_values else 0, n_values)
    eng.eng.sync()
    return out


_REFS = {}


def _ref(name, precision, pairs, Q, conditional, n_values=0):
    """The numpy path on the keys the engine holds, and the same with |values| (for the bound)."""
    key = (name, precision, tuple(pairs), Q, conditional, n_values)
    if key not in _REFS:
        b, extra, vals = _panel(name)
        f = b["individual_features"]
        keys = (_bf16_round(f) if precision == "bf16" else f).numpy().astype(np.float32)
        if extra is not None:
            keys = np.concatenate([keys, np.moveaxis(extra, 0, 2)], axis=2)
        v = np.concatenate([b["returns"].numpy().astype(np.float32)[:, :, None],
                            np.moveaxis(vals[:n_values], 0, 2)], axis=2)
        m = b["mask"].numpy()
        _REFS[key] = (sp.double_sort_numpy(keys, pairs, m, v, Q, conditional),
                      sp.double_sort_numpy(keys, pairs, m, np.abs(v), Q, conditional)["sum"])
    return _REFS[key]


def _check(got, ref, absum, mask):
    """Exact counts and breakpoints, sums within the fp64 accumulation bound; returns the largest
    deviation as a share of the bound."""
    cnt, sm = np.asarray(got["count"]), np.asarray(got["sum"])
    ba, bb = np.asarray(got["breaks_a"]), np.asarray(got["breaks_b"])
    assert cnt.dtype == np.int32 and sm.dtype == np.float64 and ba.dtype == np.float32 and bb.dtype == np.float32
    assert cnt.shape == ref["count"].shape and sm.shape == ref["sum"].shape
    np.testing.assert_array_equal(cnt, ref["count"])
    for g, r in ((ba, ref["breaks_a"]), (bb, ref["breaks_b"])):
        r = np.ascontiguousarray(r.astype(np.float32))
        assert g.shape == r.shape
        # bit for bit where finite (the sign of a zero included), NaN where numpy has NaN
        assert (np.isnan(g) == np.isnan(r)).all()
        np.testing.assert_array_equal(np.where(np.isnan(r), 0, g.view(np.uint32)), np.where(np.isnan(r), 0, r.view(np.uint32)))
    nt = mask.sum(1).astype(np.float64)
    assert (cnt.sum((-1, -2)) == nt[:, None]).all()
    assert int(got["rows"]) == int(mask.sum())
    bound = nt[:, None, None, None, None] * 2.0 ** -52 * absum + np.spacing(np.abs(ref["sum"]))
    dev = np.abs(sm - ref["sum"])
    worst = float((dev / bound).max()) if dev.size else 0.0
    print(f"largest |sum - numpy| / bound = {worst:.3f}, largest |sum - numpy| = {dev.max() if dev.size else 0.0:.3e}")
    assert (dev <= bound).all()
    return worst


@pytest.mark.parametrize("conditional", [True, False])
@pytest.mark.parametrize("Q", SHAPES)
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_panel_a_matches_numpy(precision, Q, conditional):
    mask = _panel("A")[0]["mask"].numpy()
    got = _run("A", precision, PAIRS_A, Q, conditional)
    ref, absum = _ref("A", precision, PAIRS_A, Q, conditional)
    _check(got, ref, absum, mask)
    cnt, bb = np.asarray(got["count"]), np.asarray(got["breaks_b"])
    assert (cnt[5] == 0).all() and np.isnan(np.asarray(got["breaks_a"])[5]).all() and np.isnan(bb[5]).all()
    assert (np.asarray(got["sum"])[5] == 0).all()
    live = [t for t in range(12) if t != 5]
    # the constant first key (pair 0): every row in bucket 0, the other rows of cells empty
    assert (cnt[:, 0, 0].sum(-1) == mask.sum(1)).all() and (cnt[:, 0, 1:] == 0).all()
    if conditional:
        assert np.isnan(bb[live][:, 0, 1:]).all() and np.isfinite(bb[live][:, 0, 0]).all()
        if Q == (5, 5):                                  # period 2: n_a in {1, 2} < Qb
            na = cnt[2, 4].sum(-1)
            assert set(na.tolist()) <= {1, 2} and na.sum() == 7 and ((cnt[2, 4] > 0).sum(-1) == na).all()
    else:
        assert np.isfinite(bb[live]).all()
        assert (bb[live] == bb[live][:, :, :1]).all()
    assert float(got["gpu_ms"]) > 0


@pytest.mark.parametrize("conditional", [True, False])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_panel_b_long_periods_mixed_widths_and_values(precision, conditional):
    mask = _panel("B")[0]["mask"].numpy()
    Q = (5, 5)
    got = _run("B", precision, PAIRS_B, Q, conditional, n_values=2)
    ref, absum = _ref("B", precision, PAIRS_B, Q, conditional, n_values=2)
    _check(got, ref, absum, mask)
    cnt = np.asarray(got["count"])
    assert np.asarray(got["sum"]).shape == (3, len(PAIRS_B), 5, 5, 3)
    if conditional:
        # a tie-free second key: every cell of a row holds floor or ceil of n_a / Qb rows
        # (pairs 0, 3, 4, 5); with a tie-free first key too, n_a = 520 and every cell 104
        na = cnt.sum(-1, keepdims=True)
        for p in (0, 3, 4, 5):
            assert (cnt[:, p] >= na[:, p] // 5).all() and (cnt[:, p] <= -(-na[:, p] // 5)).all()
        assert (cnt[:, 3:] == 104).all()


@pytest.mark.parametrize("Q", [(4, 9), (16, 2), (2, 16)])
def test_panel_b_other_shapes(Q):
    mask = _panel("B")[0]["mask"].numpy()
    got = _run("B", "bf16", PAIRS_B[:3], Q, True, n_values=1)
    ref, absum = _ref("B", "bf16", PAIRS_B[:3], Q, True, n_values=1)
    _check(got, ref, absum, mask)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_independent_marginals_equal_the_single_sort_kernel(precision):
    eng = _engine("A", precision)[0]
    Qa, Qb = 5, 7
    got = _run("A", precision, PAIRS_A, (Qa, Qb), conditional=False)
    cond = _run("A", precision, PAIRS_A, (Qa, Qb), conditional=True)
    cnt, ba, bb = np.asarray(got["count"]), np.asarray(got["breaks_a"]), np.asarray(got["breaks_b"])
    for p, (ca, cb) in enumerate(PAIRS_A):
        one = eng.eng.sorted_portfolios(0, Qa, [ca])
        assert np.ascontiguousarray(cnt[:, p].sum(-1)).astype(np.int32).tobytes() == np.asarray(one["count"])[:, 0].tobytes()
        assert np.ascontiguousarray(ba[:, p]).tobytes() == np.ascontiguousarray(np.asarray(one["breaks"])[:, 0]).tobytes()
        # (the conditional sort has the same first key)
        assert np.ascontiguousarray(np.asarray(cond["breaks_a"])[:, p]).tobytes() == np.ascontiguousarray(ba[:, p]).tobytes()
        assert (np.asarray(cond["count"])[:, p].sum(-1) == cnt[:, p].sum(-1)).all()
        two = eng.eng.sorted_portfolios(0, Qb, [cb])
        assert np.ascontiguousarray(cnt[:, p].sum(-2)).astype(np.int32).tobytes() == np.asarray(two["count"])[:, 0].tobytes()
        assert np.ascontiguousarray(bb[:, p, 0]).tobytes() == np.ascontiguousarray(np.asarray(two["breaks"])[:, 0]).tobytes()
    eng.eng.sync()


@pytest.mark.parametrize("conditional", [True, False])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_repeatable_and_independent_of_the_models(precision, conditional):
    a = _run("A", precision, PAIRS_A, (5, 5), conditional, n_values=2)
    b2 = _run("A", precision, PAIRS_A, (5, 5), conditional, n_values=2)
    c = _run("A", precision, PAIRS_A, (5, 5), conditional, G=3, n_values=2)
    for k in ("count", "sum", "breaks_a", "breaks_b"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b2[k]).tobytes()
        assert np.asarray(a[k]).tobytes() == np.asarray(c[k]).tobytes()
    ref, absum = _ref("A", precision, PAIRS_A, (5, 5), conditional, n_values=2)
    _check(a, ref, absum, _panel("A")[0]["mask"].numpy())


def test_pair_order_and_subsets_equal_slices():
    full = _run("A", "bf16", PAIRS_A, (5, 5))
    sel = [4, 0, 2]
    sub = _run("A", "bf16", [PAIRS_A[i] for i in sel], (5, 5))
    for k in ("count", "sum", "breaks_a", "breaks_b"):
        assert np.asarray(sub[k]).tobytes() == np.ascontiguousarray(np.asarray(full[k])[:, sel]).tobytes()


@pytest.mark.parametrize("conditional", [True, False])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_wide_path_engine(precision, conditional):
    mask = _panel("W")[0]["mask"].numpy()
    pairs = [(0, 129), (128, 64), (77, 77)]
    got = _run("W", precision, pairs, (5, 5), conditional, n_values=1)
    ref, absum = _ref("W", precision, pairs, (5, 5), conditional, n_values=1)
    _check(got, ref, absum, mask)
    assert np.asarray(got["count"]).shape == (4, 3, 5, 5)


def test_bad_arguments():
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
    b, _, vals = _panel("A")
    eng = GANEngine(_spec(46), 1, max_epochs=4)
    eng.set_data(b)
    vv = torch.zeros(3, 12, 150, device="cuda")
    torch.cuda.synchronize()
    e = eng.eng
    for kw in (dict(qa=1), dict(qb=1), dict(qa=17, qb=2), dict(qa=2, qb=17), dict(qa=6, qb=7), dict(qa=4, qb=10),
               dict(pairs=[(46, 0)]), dict(pairs=[(0, 46)]), dict(pairs=[(-1, 0)]), dict(pairs=[(0, -1)]),
               dict(pairs=[(0, 47)], extra_keys=vv.data_ptr(), n_extra=1),
               dict(values=vv.data_ptr(), n_values=3), dict(n_values=-1), dict(n_values=1), dict(n_extra=1), dict(s=3), dict(s=-1)):
        with pytest.raises(ValueError):
            e.double_sorted_portfolios(**{"s": 0, "pairs": [(0, 1)], **kw})
    with pytest.raises(RuntimeError):
        e.double_sorted_portfolios(1, [(0, 1)])           # split not set
    ok = e.double_sorted_portfolios(0, [(45, 0)], qa=2, qb=2)
    assert np.asarray(ok["count"]).shape == (12, 1, 2, 2)
    ok = e.double_sorted_portfolios(0, [(46, 0)], extra_keys=vv.data_ptr(), n_extra=1)   # defaults: 5 x 5, conditional
    assert np.asarray(ok["count"]).shape == (12, 1, 5, 5) and np.asarray(ok["breaks_b"]).shape == (12, 1, 5, 4)
    none = e.double_sorted_portfolios(0, [], qa=3, qb=4, n_values=0)
    assert np.asarray(none["count"]).shape == (12, 0, 3, 4) and np.asarray(none["sum"]).shape == (12, 0, 3, 4, 1)
    assert np.asarray(none["breaks_a"]).shape == (12, 0, 2) and np.asarray(none["breaks_b"]).shape == (12, 0, 3, 3)
    assert float(none["gpu_ms"]) == 0.0
    e.sync()


def test_python_api_cuda_matches_cpu():
    """One ensemble weight handed to both devices (evaluated by the engine): counts are equal once
    the CPU path sorts the bf16-rounded characteristics, and the priced results agree to 1e-9."""
    b = _panel("A")[0]
    models = []
    cfg = default_cli_config(8, 46, hidden_dim=[64, 64], rnn_dim=[4], dropout=0.05)
    for g in range(2):
        torch.manual_seed(100 + g)
        models.append(AssetPricingGAN(cfg).eval())
    w = sp._gpu_weights(models, b).cpu().numpy()
    br = dict(b)
    br["individual_features"] = _bf16_round(b["individual_features"])
    pairs = [(3, 4), ("weight", 7), (9, 46), (1, 2)]
    r, m = b["returns"].numpy(), b["mask"].numpy()
    for conditional in (True, False):
        gpu = sp.double_sorted_portfolios(models, b, pairs, device="cuda", weights=w, conditional=conditional)
        cpu = sp.double_sorted_portfolios(models, br, pairs, device="cpu", weights=w, conditional=conditional)
        assert gpu["names"] == cpu["names"] == ["x3 x x4", "weight x x7", "x9 x weight", "x1 x x2"]
        assert gpu["pairs"] == cpu["pairs"] and gpu["mode"] == cpu["mode"] and "gpu_ms" in gpu and "gpu_ms" not in cpu
        np.testing.assert_array_equal(gpu["count"], cpu["count"])
        np.testing.assert_array_equal(gpu["breaks_a"], cpu["breaks_a"])
        np.testing.assert_array_equal(gpu["breaks_b"], cpu["breaks_b"])
        pg, pc = sp.price_double_sorted(gpu, w, r, m), sp.price_double_sorted(cpu, w, r, m)
        for k in ("mean_ret", "alpha", "t_alpha", "ev_asset", "pair_ev", "pair_xs_r2", "pair_mean_abs_alpha", "hml",
                  "hml_sharpe", "ev", "xs_r2", "mean_abs_alpha"):
            np.testing.assert_allclose(np.asarray(pg[k]), np.asarray(pc[k]), rtol=1e-9, atol=0, equal_nan=True, err_msg=k)
    f32 = sp.double_sorted_portfolios(models, b, pairs, device="cuda", weights=w, precision="fp32")
    ex = sp.double_sorted_portfolios(models, b, pairs, device="cpu", weights=w)
    np.testing.assert_array_equal(f32["count"], ex["count"])


def test_evaluate_ensemble_end_to_end(shipped_data, capsys):
    """``double_sorts`` on both devices: the same report layout and assets, the rest of the result
    unchanged. (The numbers differ by the towers' precision and by the rows the bf16 panel moves
    across a breakpoint, so only the structure is compared.)"""
    import os
    import golden_cases as gc
    from deeplearninginassetpricing_paperreplication_amd.analysis import ensemble as ens
    ckpts = [gc.path(os.path.join("ensemble_ckpt", f"m{seed}")) for seed in (1, 2)]
    plain = ens.evaluate_ensemble(ckpts, shipped_data, device="cuda", verbose=False)
    capsys.readouterr()
    gpu = ens.evaluate_ensemble(ckpts, shipped_data, device="cuda", verbose=True, double_sorts="0:1,weight:3")
    tg = capsys.readouterr().out
    cpu = ens.evaluate_ensemble(ckpts, shipped_data, device="cpu", verbose=True, double_sorts="0:1,weight:3")
    tc = capsys.readouterr().out
    head = "DOUBLE-SORTED PORTFOLIOS"
    print(tg[tg.index(head):])
    print(tc[tc.index(head):])
    assert set(gpu) == set(plain) | {"double_sorts"}
    for k in plain:
        assert gpu[k] == plain[k]
    g, c = gpu["double_sorts"], cpu["double_sorts"]
    assert "gpu_ms" in g["portfolios"] and "gpu_ms" not in c["portfolios"]
    assert g["portfolios"]["names"] == c["portfolios"]["names"] and len(g["portfolios"]["names"]) == 2
    assert g["portfolios"]["pairs"] == c["portfolios"]["pairs"] == [(0, 1), (46, 3)]
    assert g["portfolios"]["count"].shape == c["portfolios"]["count"].shape == (60, 2, 5, 5)
    np.testing.assert_array_equal(g["portfolios"]["count"].sum((-1, -2)), c["portfolios"]["count"].sum((-1, -2)))
    assert set(g["priced"]) == set(c["priced"])
    assert g["priced"]["assets"] == c["priced"]["assets"] == 50
    assert np.isfinite(g["priced"]["hml"]).all() and np.isfinite(g["priced"]["ev"]) and np.isfinite(g["priced"]["pair_ev"]).all()
    assert len(tg[tg.index(head):].splitlines()) == len(tc[tc.index(head):].splitlines())
