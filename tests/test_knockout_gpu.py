"""The knock-out kernels (``csrc/k_knock.hip``, ``Engine.knockout``) on a real MI355X.

Reference ops: ``forward_split`` on a panel uploaded with the scenario's columns overwritten (the
tower pass, bit for bit), ``analysis.knockout.knockout_sums_numpy`` (the reduction) and the CPU path
of ``knockout_importance`` (end to end). The panel is the one of ``test_importance_gpu.py``: 12 x 150,
M = 8, masked stocks, an empty period, R = 11 * 129 = 1419 rows -- 45 tiles, the last one ragged,
three workgroups of ``k_knock_fwd`` with the last one partial."""
import numpy as np
import pytest
import torch

from deeplearninginassetpricing_paperreplication_amd.analysis import knockout as ko
from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config
from deeplearninginassetpricing_paperreplication_amd.data.synthetic import generate_panel_fast
from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN

pytestmark = pytest.mark.gpu

G = 3
SUMS = ("EA", "E2", "ER", "S1", "SA", "SR")
PER = ("n", "sum_r", "sum_rr")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeplearninginassetpricing_paperreplication_amd.ops import native
    native.load(required=True)


_PANELS = {}


def _batch(F=46):
    if F not in _PANELS:
        ret, feats, mask, mac = generate_panel_fast(12, 150, F, 8, seed=0)
        mac = (mac - mac.mean(0)) / (mac.std(0, unbiased=False) + 1e-8)
        mask = mask.clone()
        mask[:, torch.arange(150) % 7 == 3] = False  # masked stocks
        mask[5] = False                              # an empty period
        assert int(mask.sum()) == 11 * 129
        _PANELS[F] = {"returns": ret, "individual_features": feats, "mask": mask, "macro_features": mac}
    return _PANELS[F]


# name -> (F, config keywords)
ARCHS = {
    "h64x2_r4": (46, dict(hidden_dim=[64, 64], rnn_dim=[4])),
    "h64x4_r4": (46, dict(hidden_dim=[64] * 4, rnn_dim=[4])),
    "h48_32_r2x2": (46, dict(hidden_dim=[48, 32], rnn_dim=[2, 2])),
    "no_rnn": (46, dict(hidden_dim=[64, 64], use_lstm=False)),
    "F20": (20, dict(hidden_dim=[64, 64], rnn_dim=[4])),
}


def _models(name, n=G, **extra):
    F, kw = ARCHS[name]
    cfg = dict(default_cli_config(8, F, dropout=0.05, **kw), **extra)
    out = []
    for g in range(n):
        torch.manual_seed(100 + g)
        out.append(AssetPricingGAN(cfg).eval())
    return out


def _base_and_scenarios(F):
    """A base row with 0 and values bf16 cannot represent, and the scenarios {}, {0}, {F-1}, a
    5-column group (it crosses the 32-column k-step of the 46-column panels)."""
    group = (1, 9, 17, 33, 41) if F == 46 else (1, 5, 9, 13, 17)
    base = np.zeros(F)
    base[[0, F - 1]] = 0.3, -0.7
    base[list(group)] = 0.3, -0.7, 0.0, 0.3, -0.7
    return base, [(), (0,), (F - 1,), group]


def _engine(models, b, precision="bf16"):
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
    eng = GANEngine(models[0].spec, len(models), max_epochs=4, precision=precision)
    eng.set_data(b)
    for g, m in enumerate(models):
        eng.set_model(g, m, 0)
    return eng


def _run(eng, n_models, cols, base, dense=False, raw=False, raw_in=None, max_scratch_bytes=0):
    """Engine.knockout as numpy arrays; dense [K][T][N] / raw [K][G][R] when asked for."""
    sp = eng.splits[0]
    F, K = eng.spec.individual_dim, len(cols)
    wd = torch.zeros(K, sp.T, sp.N, dtype=torch.float32, device="cuda") if dense else None
    rw = torch.full((K, n_models, sp.R), float("nan"), dtype=torch.float32, device="cuda") if raw else None
    ri = None if raw_in is None else torch.as_tensor(raw_in, dtype=torch.float32).cuda().contiguous()
    assert ri is None or tuple(ri.shape) == (K, n_models, sp.R)
    torch.cuda.synchronize()
    r = eng.eng.knockout(0, ko.scenario_masks(cols, F), K, [float(x) for x in np.asarray(base, dtype=np.float32)],
                         wd.data_ptr() if dense else 0, True, max_scratch_bytes, rw.data_ptr() if raw else 0,
                         ri.data_ptr() if ri is not None else 0)
    eng.eng.sync()
    out = {k: np.asarray(r[k]) for k in SUMS + PER}
    out["chunks"], out["rows"] = int(r["chunks"]), int(r["rows"])
    if dense:
        out["dense"] = wd.cpu().numpy()
    if raw:
        out["raw"] = rw.cpu().numpy()
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert (_bits(a) == _bits(b)).all(), what


def _dense_rows(wc, mask):
    """[.., R] compact rows (period-major, stocks ascending) as [.., T, N], zero elsewhere."""
    out = np.zeros(wc.shape[:-1] + mask.shape, dtype=wc.dtype)
    out[..., mask] = wc
    return out


def _overwritten(b, cols, base):
    b2 = dict(b)
    x = b["individual_features"].clone()
    if len(cols):
        x[:, :, list(cols)] = torch.as_tensor(np.asarray(base, dtype=np.float32)[list(cols)])
    b2["individual_features"] = x
    return b2


def _magnitudes(w64, ret, mask, norm):
    """Sum of the magnitudes of the terms of each sum ([K][G][T] or [K][T]) from float64 raw weights
    [K][G][T][N]: a term of v is |w| + |c|, a term of e that times the member's scale."""
    md = mask.astype(np.float64)
    n = np.maximum(md.sum(1), 1.0)
    aw = np.abs(w64) * md
    s64 = ko.knockout_sums_numpy(w64, ret, mask, norm, np.float64)
    c = np.abs(s64["S1"] / n) if norm else np.zeros_like(s64["S1"])
    a = (np.abs(w64) + c[..., None]) * md
    sc = 1.0 / (w64.shape[1] * np.maximum(s64["SA"], 1e-8))
    ae = (a * sc[..., None]).sum(1)                                       # [K][T][N] >= |e|
    R = np.abs(np.where(mask, ret, 0.0)).astype(np.float64)
    return s64, {"S1": aw.sum(3), "SA": a.sum(3), "SR": (a * R).sum(3), "EA": ae.sum(2), "ER": (ae * R).sum(2),
                 "E2": 2.0 * (ae * ae).sum(2)}


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name", list(ARCHS))
def test_tower_bits_equal_the_forward_on_an_overwritten_panel(name, precision):
    F = ARCHS[name][0]
    b, models = _batch(F), _models(name)
    base, cols = _base_and_scenarios(F)
    mask, ret = b["mask"].numpy(), b["returns"].numpy()
    A = _engine(models, b, precision)
    got = _run(A, G, cols, base, dense=True, raw=True)
    assert got["rows"] == 1419 and np.isfinite(got["raw"]).all()
    for k, cs in enumerate(cols):
        B = _engine(models, _overwritten(b, cs, base), precision)
        B.eng.forward_split(0, False, False)
        w = torch.empty(G, 1419, dtype=torch.float32, device="cuda")
        for g in range(G):
            assert B.eng.copy_ws(g, 0, "w", w[g].data_ptr()) == 1419
        B.eng.sync()
        w = w.cpu().numpy()
        _same_bits(got["raw"][k], w, f"raw weights, scenario {k}")
        # the same reduction on the second engine's raw weights: its baseline scenario
        ref = _run(B, G, [()], base, dense=True, raw=True)
        _same_bits(ref["raw"][0], w, f"baseline of the overwritten panel, scenario {k}")
        for key in SUMS:
            _same_bits(got[key][k], ref[key][0], f"{key}, scenario {k}")
        _same_bits(got["dense"][k], ref["dense"][0], f"dense, scenario {k}")
        # member sums and the dense weights from that w in numpy, with the stated roundings: fp64 sums
        # of at most 129 terms in another order differ by at most 129 * 2^-53 of the terms' magnitudes
        s32 = ko.knockout_sums_numpy(_dense_rows(w, mask)[None], ret, mask, True, np.float32, dense=True)
        _, mg = _magnitudes(_dense_rows(w.astype(np.float64), mask)[None], ret, mask, True)
        for key in ("S1", "SA", "SR"):
            assert (np.abs(got[key][k] - s32[key][0]) <= 129 * 2.0 ** -53 * mg[key][0]).all(), (key, k)
        np.testing.assert_allclose(got["dense"][k], s32["dense"][0], rtol=2.0 ** -22, atol=0)
        del B
    for key in PER:
        np.testing.assert_array_equal(got[key][5], 0.0)
    assert (got["n"] == mask.sum(1)).all()
    for k in (1, 2, 3):
        assert (got["raw"][0] != got["raw"][k]).any()


@pytest.mark.parametrize("name,precision", [("h64x2_r4", "fp32"), ("h64x2_r4", "bf16"), ("F20", "fp32")])
def test_reduction_against_float64_numpy(name, precision):
    """EA, E2, ER, SA, SR, S1 within (G + 3) * 2^-24 of the summed magnitudes of their terms: the
    fp32 roundings of c, v, the scale and the G fmas, each relative to a term (|w| + |c|, times the
    scale for e; E2's terms are 2 |e| |delta e|)."""
    F = ARCHS[name][0]
    b, models = _batch(F), _models(name)
    base, cols = _base_and_scenarios(F)
    mask, ret = b["mask"].numpy(), b["returns"].numpy()
    got = _run(_engine(models, b, precision), G, cols, base, raw=True)
    w64 = _dense_rows(got["raw"].astype(np.float64), mask)
    s64, mg = _magnitudes(w64, ret, mask, True)
    for key in SUMS:
        err = np.abs(got[key] - s64[key])
        print(f"{name} {precision} {key}: max err / bound {np.max(err / np.maximum((G + 3) * 2.0 ** -24 * mg[key], 1e-300)):.3e}")
        assert (err <= (G + 3) * 2.0 ** -24 * mg[key]).all(), key
    for key in PER:
        np.testing.assert_allclose(got[key], s64[key], rtol=1e-13, atol=0)


def test_integer_weights_sum_exactly_without_normalisation():
    models = _models("h64x2_r4", normalize_w=False)
    b = _batch()
    mask, ret = b["mask"].numpy(), b["returns"].numpy()
    rng = np.random.default_rng(3)
    wi = rng.integers(-1000, 1001, size=(2, G, 1419)).astype(np.float32)
    got = _run(_engine(models, b), G, [(), (0,)], np.zeros(46), raw_in=wi)
    wd = _dense_rows(wi.astype(np.float64), mask)
    np.testing.assert_array_equal(got["S1"], wd.sum(3))
    np.testing.assert_array_equal(got["SA"], np.abs(wd).sum(3))          # c = 0: v = w
    s64, mg = _magnitudes(wd, ret, mask, False)
    for key in SUMS:
        assert (np.abs(got[key] - s64[key]) <= (G + 3) * 2.0 ** -24 * mg[key]).all(), key
    # with the normalisation the same weights give another SA
    norm = _run(_engine(_models("h64x2_r4"), b), G, [(), (0,)], np.zeros(46), raw_in=wi)
    np.testing.assert_array_equal(norm["S1"], got["S1"])
    assert (norm["SA"] != got["SA"]).any()


def test_outputs_do_not_depend_on_position_chunking_or_company():
    F = 46
    b, models = _batch(F), _models("h64x2_r4")
    base, four = _base_and_scenarios(F)
    cols = four + [(2,), (31, 32), (45, 0), tuple(range(0, 46, 3)), tuple(range(46))]
    assert len(cols) == 9
    eng = _engine(models, b)
    full = _run(eng, G, cols, base, dense=True)
    again = _run(eng, G, cols, base, dense=True)
    one = _run(eng, G, cols, base, dense=True, max_scratch_bytes=1)
    assert full["chunks"] == 1 and one["chunks"] == 9
    rev = _run(eng, G, cols[::-1], base, dense=True)
    for key in SUMS + ("dense",):
        _same_bits(full[key], again[key], key)
        _same_bits(full[key], one[key], key)
        _same_bits(full[key], rev[key][::-1], key)
    for key in PER:
        _same_bits(full[key], one[key], key)
        _same_bits(full[key], rev[key], key)
    for k in (0, 3, 8):
        solo = _run(eng, G, [cols[k]], base, dense=True)
        for key in SUMS + ("dense",):
            _same_bits(full[key][k], solo[key][0], (key, k))
    # a member alone and batched with two others
    for g in range(G):
        alone = _run(_engine([models[g]], b), 1, cols, base)
        for key in ("S1", "SA", "SR"):
            _same_bits(full[key][:, g], alone[key][:, 0], (key, g))


_CPU = {}


def _cpu_report(name):
    if name not in _CPU:
        F = ARCHS[name][0]
        _CPU[name] = ko.knockout_importance(_models(name), _batch(F), groups={"grp": list(_base_and_scenarios(F)[1][3])},
                                            base=_base_and_scenarios(F)[0], xs_r2=True, dtype=torch.float32)
    return _CPU[name]


@pytest.mark.parametrize("name", list(ARCHS))
def test_fp32_engine_matches_the_float32_cpu_path(name, capsys):
    F = ARCHS[name][0]
    cpu = _cpu_report(name)
    got = ko.knockout_importance(_models(name), _batch(F), groups={"grp": list(_base_and_scenarios(F)[1][3])},
                                 base=_base_and_scenarios(F)[0], xs_r2=True, device="cuda", precision="fp32")
    assert "using the CPU path" not in capsys.readouterr().out
    assert got["path"] == "engine" and cpu["path"] == "cpu" and got["scenarios"] == cpu["scenarios"]
    assert len(got["scenarios"]) == 1 + F + 1
    scale = np.abs(cpu["factor"]).max()
    err = np.abs(got["factor"] - cpu["factor"]).max(1) / scale
    print(f"fp32 {name}: max |dF| / max |F| = {err.max():.3e} (scenario {int(err.argmax())}); "
          f"max |d sharpe| {np.abs(got['sharpe'] - cpu['sharpe']).max():.3e}, max |d ev| {np.abs(got['ev'] - cpu['ev']).max():.3e}, "
          f"max |d xs_r2| {np.abs(got['xs_r2'] - cpu['xs_r2']).max():.3e}")
    assert (err <= 1e-5).all(), err.max()       # the project's fp32 acceptance bound


def _spearman(a, b):
    ra, rb = np.argsort(np.argsort(a)).astype(np.float64), np.argsort(np.argsort(b)).astype(np.float64)
    return float(np.corrcoef(ra, rb)[0, 1])


def test_bf16_engine_ranks_like_fp32(capsys):
    name = "h64x2_r4"
    kw = dict(groups={"grp": [1, 9, 17, 33, 41]}, device="cuda")
    lo = ko.knockout_importance(_models(name), _batch(), precision="bf16", **kw)
    hi = ko.knockout_importance(_models(name), _batch(), precision="fp32", **kw)
    assert "using the CPU path" not in capsys.readouterr().out
    rho = _spearman(lo["d_sharpe"][1:], hi["d_sharpe"][1:])
    print(f"bf16 vs fp32 {name}: Spearman of d_sharpe {rho:.4f}, max |d sharpe| {np.abs(lo['sharpe'] - hi['sharpe']).max():.3e}, "
          f"max |d ev| {np.abs(lo['ev'] - hi['ev']).max():.3e}")
    assert rho > 0


def _assert_cpu_numbers(got, ref):
    assert got["path"] == "cpu"
    for k in ("sharpe", "ev", "member_sharpes", "factor", "d_sharpe"):
        np.testing.assert_array_equal(got[k], ref[k])


def test_wide_path_is_not_covered_and_falls_back(monkeypatch, capsys):
    name = "h64x2_r4"
    b, models = _batch(), _models(name)
    ref = ko.knockout_importance(models, b, singles=False, groups={"g": [0, 1]})
    monkeypatch.setenv("DLAP_WIDE", "1")
    eng = _engine(models, b)
    assert int(eng.desc["wide"]) == 1 and not eng.eng.knockout_supported()
    with pytest.raises(ValueError, match="knockout: not available"):
        _run(eng, G, [()], np.zeros(46))
    eng.eng.sync()
    del eng
    capsys.readouterr()
    got = ko.knockout_importance(models, b, singles=False, groups={"g": [0, 1]}, device="cuda")
    assert "using the CPU path" in capsys.readouterr().out
    _assert_cpu_numbers(got, ref)
    monkeypatch.delenv("DLAP_WIDE")
    assert _engine(models, b).eng.knockout_supported()


def test_mixed_architectures_fall_back(capsys):
    b = _batch()
    models = _models("h64x2_r4", 2) + _models("h64x4_r4", 1)
    ref = ko.knockout_importance(models, b, singles=False, groups={"g": [0, 1]})
    got = ko.knockout_importance(models, b, singles=False, groups={"g": [0, 1]}, device="cuda")
    assert "mixed-architecture ensemble: using the CPU path" in capsys.readouterr().out
    _assert_cpu_numbers(got, ref)


def test_argument_errors():
    b, models = _batch(), _models("no_rnn", 1)
    eng = _engine(models, b)
    m = ko.scenario_masks([()], 46)
    base = [0.0] * 46
    bad = m.copy()
    bad[0, 1] = np.uint32(1 << 14)                                   # column 46
    with pytest.raises(ValueError, match="column outside"):
        eng.eng.knockout(0, bad, 1, base)
    with pytest.raises(ValueError, match="masks"):
        eng.eng.knockout(0, m, 2, base)
    with pytest.raises(ValueError, match="base"):
        eng.eng.knockout(0, m, 1, base[:-1])
    with pytest.raises(ValueError, match="split"):
        eng.eng.knockout(1, m, 1, base)
    with pytest.raises(ValueError, match="outside"):
        ko.knockout_importance(models, b, groups={"g": [46]}, device="cuda")
    eng.eng.sync()
    # more periods than the panel launchers accept: the engine refuses such a split when it is set
    # (its own limit is lower), so the error comes before Engine.knockout's own check of T <= 65535
    Tl = 65536
    g = torch.Generator().manual_seed(1)
    long = {"returns": torch.zeros(Tl, 2), "individual_features": torch.rand(Tl, 2, 46, generator=g) - 0.5,
            "mask": torch.ones(Tl, 2, dtype=torch.bool), "macro_features": torch.zeros(Tl, 8)}
    with pytest.raises(ValueError):
        big = _engine(models, long)
        big.eng.knockout(0, m, 1, base)
    with pytest.raises(ValueError):
        ko.knockout_importance(models, long, singles=False, device="cuda")


def test_evaluate_ensemble_end_to_end(shipped_data, capsys):
    import os

    import golden_cases as gc
    from deeplearninginassetpricing_paperreplication_amd.analysis import ensemble as ens
    ckpts = [gc.path(os.path.join("ensemble_ckpt", f"m{seed}")) for seed in (1, 2)]
    plain = ens.evaluate_ensemble(ckpts, shipped_data, device="cuda", verbose=False)
    kw = dict(verbose=False, knockout=True, knockout_groups={"first": [0, 1, 2]}, knockout_xs_r2=True)
    gpu = ens.evaluate_ensemble(ckpts, shipped_data, device="cuda", **kw)
    assert "using the CPU path" not in capsys.readouterr().out
    cpu = ens.evaluate_ensemble(ckpts, shipped_data, device="cpu", **kw)
    for k in plain:
        assert gpu[k] == plain[k], k
    a, c = gpu["knockout"], cpu["knockout"]
    assert a["path"] == "engine" and c["path"] == "cpu" and a["scenarios"] == c["scenarios"]
    assert a["scenarios"][-1] == "first" and len(a["scenarios"]) == 48
    # the bf16 engine against float32 torch: the project's bf16 bound on the factor series
    err = np.abs(a["factor"] - c["factor"]).max() / np.abs(c["factor"]).max()
    rho = _spearman(a["d_sharpe"][1:], c["d_sharpe"][1:])
    print(f"end to end: max |dF| / max |F| {err:.3e}, Spearman of d_sharpe {rho:.4f}, "
          f"baseline Sharpe {a['sharpe'][0]:.4f} / {c['sharpe'][0]:.4f}")
    assert err < 0.08 and rho > 0
    assert abs(a["sharpe"][0] - plain["test_sharpe"]) <= 1e-5
