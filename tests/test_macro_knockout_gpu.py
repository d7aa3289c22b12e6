"""Macro knock-outs (``k_knock_macro_fill`` / ``k_knock_fwd_pp`` in ``csrc/k_knock.hip``,
``Engine.knockout_macro``) on a real MI355X.

Reference ops: ``forward_split`` on a split uploaded with the scenario's macro and characteristic
columns overwritten (the recurrence and the tower pass, bit for bit), ``Engine.knockout`` (the
reduction, and the scenarios without a macro set) and the CPU path of ``knockout_importance`` (end to
end). Panels: the 12 x 150 panel of ``test_knockout_gpu.py`` (M = 8, masked stocks, an empty period,
1419 rows: 45 tiles, the last one ragged) and the same recipe with 20 periods (1761 rows: 56 tiles, the
last one holding one row; two 16-period projection tiles, the second ragged)."""
import numpy as np
import pytest
import torch

from deeplearninginassetpricing_paperreplication_amd.analysis import knockout as ko
from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config
from deeplearninginassetpricing_paperreplication_amd.data.synthetic import generate_panel_fast
from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN

pytestmark = pytest.mark.gpu

G, M = 3, 8
SUMS = ("EA", "E2", "ER", "S1", "SA", "SR")
PER = ("n", "sum_r", "sum_rr")
ROWS = {12: 1419, 20: 1761}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeplearninginassetpricing_paperreplication_amd.ops import native
    native.load(required=True)


_PANELS = {}


def _batch(F=46, T=12):
    if (F, T) not in _PANELS:
        ret, feats, mask, mac = generate_panel_fast(T, 150, F, M, seed=0)
        mac = (mac - mac.mean(0)) / (mac.std(0, unbiased=False) + 1e-8)
        mask = mask.clone()
        mask[:, torch.arange(150) % 7 == 3] = False  # masked stocks
        mask[5] = False                              # an empty period
        assert int(mask.sum()) == ROWS[T]
        _PANELS[(F, T)] = {"returns": ret, "individual_features": feats, "mask": mask, "macro_features": mac}
    return _PANELS[(F, T)]


# name -> (F, config keywords)
ARCHS = {
    "h64x2_r4": (46, dict(hidden_dim=[64, 64], rnn_dim=[4])),
    "h48_32_r2x2": (46, dict(hidden_dim=[48, 32], rnn_dim=[2, 2])),
    "no_rnn": (46, dict(hidden_dim=[64, 64], use_lstm=False)),
    "h64x2_r8": (46, dict(hidden_dim=[64, 64], rnn_dim=[8])),
    "F20": (20, dict(hidden_dim=[64, 64], rnn_dim=[4])),
}


def _models(name, n=G, **extra):
    F, kw = ARCHS[name]
    cfg = dict(default_cli_config(M, F, dropout=0.05, **kw), **extra)
    out = []
    for g in range(n):
        torch.manual_seed(100 + g)
        out.append(AssetPricingGAN(cfg).eval())
    return out


def _bases(F):
    """The characteristic base of ``test_knockout_gpu._base_and_scenarios`` and the macro base: zero
    except series 0 and 7 at values bf16 cannot represent."""
    group = (1, 9, 17, 33, 41) if F == 46 else (1, 5, 9, 13, 17)
    base = np.zeros(F)
    base[[0, F - 1]] = 0.3, -0.7
    base[list(group)] = 0.3, -0.7, 0.0, 0.3, -0.7
    mbase = np.zeros(M)
    mbase[[0, 7]] = 0.3, -0.7
    return base, mbase


# (characteristic columns, macro series)
FIVE = [((), ()), ((), (0,)), ((), (7,)), ((), (1, 3, 6)), ((0,), (2,))]
NINE = FIVE + [((), (2,)), ((), tuple(range(8))), ((31, 32), (4, 5)), ((), (0,))]


def _engine(models, b, precision="bf16"):
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
    eng = GANEngine(models[0].spec, len(models), max_epochs=4, precision=precision)
    eng.set_data(b)
    for g, m in enumerate(models):
        eng.set_model(g, m, 0)
    return eng


def _f32(x):
    return [float(v) for v in np.asarray(x, dtype=np.float32)]


def _run(eng, n_models, scen, base, mbase, dense=False, raw=False, max_scratch_bytes=0):
    """Engine.knockout_macro as numpy arrays; dense [K][T][N] / raw [K][G][R] when asked for."""
    sp = eng.splits[0]
    F, K = eng.spec.individual_dim, len(scen)
    wd = torch.zeros(K, sp.T, sp.N, dtype=torch.float32, device="cuda") if dense else None
    rw = torch.full((K, n_models, sp.R), float("nan"), dtype=torch.float32, device="cuda") if raw else None
    torch.cuda.synchronize()
    r = eng.eng.knockout_macro(0, ko.scenario_masks([c for c, _ in scen], F),
                               ko.macro_scenario_masks([q for _, q in scen], M), K, _f32(base), _f32(mbase),
                               wd.data_ptr() if dense else 0, True, max_scratch_bytes, rw.data_ptr() if raw else 0)
    eng.eng.sync()
    out = {k: np.asarray(r[k]) for k in SUMS + PER}
    for k in ("chunks", "rows", "lstm_jobs"):
        out[k] = int(r[k])
    out["ms"] = (float(r["lstm_ms"]), float(r["fwd_ms"]), float(r["reduce_ms"]))
    if dense:
        out["dense"] = wd.cpu().numpy()
    if raw:
        out["raw"] = rw.cpu().numpy()
    return out


def _run_plain(eng, n_models, cols, base, dense=False, raw=False):
    """Engine.knockout (characteristic scenarios) the same way."""
    sp = eng.splits[0]
    F, K = eng.spec.individual_dim, len(cols)
    wd = torch.zeros(K, sp.T, sp.N, dtype=torch.float32, device="cuda") if dense else None
    rw = torch.full((K, n_models, sp.R), float("nan"), dtype=torch.float32, device="cuda") if raw else None
    torch.cuda.synchronize()
    r = eng.eng.knockout(0, ko.scenario_masks(cols, F), K, _f32(base), wd.data_ptr() if dense else 0, True, 0,
                         rw.data_ptr() if raw else 0)
    eng.eng.sync()
    out = {k: np.asarray(r[k]) for k in SUMS + PER}
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


def _overwritten(b, cols, base, q, mbase):
    b2 = dict(b)
    x = b["individual_features"].clone()
    if len(cols):
        x[:, :, list(cols)] = torch.as_tensor(np.asarray(base, dtype=np.float32)[list(cols)])
    mac = b["macro_features"].clone()
    if len(q):
        mac[:, list(q)] = torch.as_tensor(np.asarray(mbase, dtype=np.float32)[list(q)])
    b2["individual_features"], b2["macro_features"] = x, mac
    return b2


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name,T", [("h64x2_r4", 12), ("h64x2_r4", 20), ("h48_32_r2x2", 20), ("no_rnn", 12),
                                    ("h64x2_r8", 20), ("F20", 12)])
def test_bits_equal_the_forward_on_an_overwritten_split(name, T, precision):
    F = ARCHS[name][0]
    b, models = _batch(F, T), _models(name)
    base, mbase = _bases(F)
    R = ROWS[T]
    A = _engine(models, b, precision)
    assert A.eng.knockout_macro_supported()
    got = _run(A, G, FIVE, base, mbase, dense=True, raw=True)
    assert got["rows"] == R and got["chunks"] == 1 and np.isfinite(got["raw"]).all()
    assert got["lstm_jobs"] == (0 if name == "no_rnn" else 4 * G)
    for k, (cs, q) in enumerate(FIVE):
        B = _engine(models, _overwritten(b, cs, base, q, mbase), precision)
        B.eng.forward_split(0, False, False)
        w = torch.empty(G, R, dtype=torch.float32, device="cuda")
        for g in range(G):
            assert B.eng.copy_ws(g, 0, "w", w[g].data_ptr()) == R
        B.eng.sync()
        w = w.cpu().numpy()
        _same_bits(got["raw"][k], w, f"raw weights, scenario {k}")
        ref = _run_plain(B, G, [()], base, dense=True, raw=True)        # the existing baseline of that engine
        _same_bits(ref["raw"][0], w, f"baseline of the overwritten split, scenario {k}")
        for key in SUMS:
            _same_bits(got[key][k], ref[key][0], f"{key}, scenario {k}")
        _same_bits(got["dense"][k], ref["dense"][0], f"dense, scenario {k}")
        del B
    assert (got["n"] == b["mask"].numpy().sum(1)).all()
    for k in (1, 2, 3, 4):
        assert (got["raw"][0] != got["raw"][k]).any(), k


@pytest.mark.parametrize("name,precision", [("h64x2_r4", "bf16"), ("no_rnn", "fp32"), ("h48_32_r2x2", "bf16")])
def test_scenarios_without_a_macro_set_equal_engine_knockout(name, precision):
    F = ARCHS[name][0]
    b, models = _batch(F, 20), _models(name)
    base, mbase = _bases(F)
    cols = [(), (0,), (F - 1,), (1, 9, 17, 33, 41), (31, 32)]
    eng = _engine(models, b, precision)
    old = _run_plain(eng, G, cols, base, dense=True, raw=True)
    new = _run(eng, G, [(c, ()) for c in cols], base, mbase, dense=True, raw=True)
    assert new["lstm_jobs"] == 0
    for key in SUMS + PER + ("dense", "raw"):
        _same_bits(new[key], old[key], key)
    # and beside scenarios that have one
    mixed = _run(eng, G, [((), (0,))] + [(c, ()) for c in cols] + [((0,), (2,))], base, mbase, dense=True, raw=True)
    for key in SUMS + ("dense", "raw"):
        _same_bits(mixed[key][1:-1], old[key], key)


def test_outputs_do_not_depend_on_position_chunking_or_company():
    F = 46
    b, models = _batch(F, 20), _models("h64x2_r4")
    base, mbase = _bases(F)
    assert len(NINE) == 9
    eng = _engine(models, b)
    full = _run(eng, G, NINE, base, mbase, dense=True)
    again = _run(eng, G, NINE, base, mbase, dense=True)
    one = _run(eng, G, NINE, base, mbase, dense=True, max_scratch_bytes=1)
    assert full["chunks"] == 1 and one["chunks"] == 9 and full["lstm_jobs"] == one["lstm_jobs"] == 8 * G
    rev = _run(eng, G, NINE[::-1], base, mbase, dense=True)
    for key in SUMS + ("dense",):
        _same_bits(full[key], again[key], key)
        _same_bits(full[key], one[key], key)
        _same_bits(full[key], rev[key][::-1], key)
        _same_bits(full[key][1], full[key][8], key)              # the repeat of Q = {0}
    for key in PER:
        _same_bits(full[key], one[key], key)
        _same_bits(full[key], rev[key], key)
    for k in (0, 3, 6, 7):
        solo = _run(eng, G, [NINE[k]], base, mbase, dense=True)
        for key in SUMS + ("dense",):
            _same_bits(full[key][k], solo[key][0], (key, k))
    # a member alone and batched with two others
    for g in range(G):
        alone = _run(_engine([models[g]], b), 1, NINE, base, mbase)
        for key in ("S1", "SA", "SR"):
            _same_bits(full[key][:, g], alone[key][:, 0], (key, g))


@pytest.mark.parametrize("name", ["h64x2_r4", "h48_32_r2x2"])
def test_a_dead_input_weight_column_changes_nothing(name):
    F = ARCHS[name][0]
    b, models = _batch(F, 20), _models(name)
    for m in models:
        with torch.no_grad():
            m.sdf_net.macro_lstm.lstm.weight_ih_l0[:, 2] = 0.0
    base = np.zeros(F)
    got = _run(_engine(models, b), G, [((), ()), ((), (2,)), ((), (3,))], base, np.full(M, 0.3), dense=True, raw=True)
    assert got["lstm_jobs"] == 2 * G
    for key in SUMS + ("dense", "raw"):
        _same_bits(got[key][1], got[key][0], key)
    assert (got["raw"][2] != got["raw"][0]).any()


_CPU = {}


def _report_kw(F):
    base, mbase = _bases(F)
    return dict(singles=False, groups={"grp": [1, 9, 17]}, base=base, macro=True, macro_groups={"mg": [1, 3, 6]},
                macro_base=mbase, extra_scenarios=[("both", [0], [2])])


def _cpu_report(name):
    if name not in _CPU:
        F = ARCHS[name][0]
        _CPU[name] = ko.knockout_importance(_models(name), _batch(F), dtype=torch.float32, **_report_kw(F))
    return _CPU[name]


@pytest.mark.parametrize("name", list(ARCHS))
def test_fp32_engine_matches_the_float32_cpu_path(name, capsys):
    F = ARCHS[name][0]
    cpu = _cpu_report(name)
    got = ko.knockout_importance(_models(name), _batch(F), device="cuda", precision="fp32", **_report_kw(F))
    assert "using the CPU path" not in capsys.readouterr().out
    assert got["path"] == "engine" and cpu["path"] == "cpu" and got["scenarios"] == cpu["scenarios"]
    assert got["scenarios"] == ["baseline", "grp"] + [f"macro{j}" for j in range(M)] + ["mg", "both"]
    assert got["macro_columns"] == cpu["macro_columns"] and got["macro_columns"][-1] == [2]
    scale = np.abs(cpu["factor"]).max()
    err = np.abs(got["factor"] - cpu["factor"]).max(1) / scale
    print(f"macro fp32 {name}: max |dF| / max |F| = {err.max():.3e} (scenario {int(err.argmax())}); "
          f"max |d sharpe| {np.abs(got['sharpe'] - cpu['sharpe']).max():.3e}, max |d ev| {np.abs(got['ev'] - cpu['ev']).max():.3e}")
    assert (err <= 1e-5).all(), err.max()       # the project's fp32 acceptance bound


def _spearman(a, b):
    ra, rb = np.argsort(np.argsort(a)).astype(np.float64), np.argsort(np.argsort(b)).astype(np.float64)
    return float(np.corrcoef(ra, rb)[0, 1])


def test_bf16_engine_ranks_like_fp32(capsys):
    name = "h64x2_r4"
    kw = dict(_report_kw(46), device="cuda")
    lo = ko.knockout_importance(_models(name), _batch(), precision="bf16", **kw)
    hi = ko.knockout_importance(_models(name), _batch(), precision="fp32", **kw)
    assert "using the CPU path" not in capsys.readouterr().out
    mk = [k for k, q in enumerate(lo["macro_columns"]) if q]
    assert len(mk) == M + 2
    rho = _spearman(lo["d_sharpe"][mk], hi["d_sharpe"][mk])
    print(f"macro bf16 vs fp32 {name}: Spearman of d_sharpe {rho:.4f}, max |d sharpe| "
          f"{np.abs(lo['sharpe'] - hi['sharpe']).max():.3e}, max |d ev| {np.abs(lo['ev'] - hi['ev']).max():.3e}, "
          f"max |dF| / max |F| {np.abs(lo['factor'] - hi['factor']).max() / np.abs(hi['factor']).max():.3e}")
    assert rho > 0


def _assert_cpu_numbers(got, ref):
    assert got["path"] == "cpu"
    for k in ("sharpe", "ev", "member_sharpes", "factor", "d_sharpe"):
        np.testing.assert_array_equal(got[k], ref[k])
    assert got["macro_columns"] == ref["macro_columns"]


def test_wide_path_is_not_covered_and_falls_back(monkeypatch, capsys):
    name = "h64x2_r4"
    b, models = _batch(), _models(name)
    kw = dict(singles=False, macro=True, macro_singles=False, macro_groups={"g": [0, 1]})
    ref = ko.knockout_importance(models, b, **kw)
    monkeypatch.setenv("DLAP_WIDE", "1")
    eng = _engine(models, b)
    assert int(eng.desc["wide"]) == 1 and not eng.eng.knockout_macro_supported()
    with pytest.raises(ValueError, match="knockout_macro: not available"):
        _run(eng, G, [((), (0,))], np.zeros(46), np.zeros(M))
    eng.eng.sync()
    del eng
    capsys.readouterr()
    got = ko.knockout_importance(models, b, device="cuda", **kw)
    assert "not available for this shape: using the CPU path" in capsys.readouterr().out
    _assert_cpu_numbers(got, ref)
    monkeypatch.delenv("DLAP_WIDE")
    assert _engine(models, b).eng.knockout_macro_supported()


def test_mixed_architectures_fall_back(capsys):
    b = _batch()
    models = _models("h64x2_r4", 2) + _models("h64x2_r8", 1)
    kw = dict(singles=False, macro=True, macro_singles=False, macro_groups={"g": [0, 1]})
    ref = ko.knockout_importance(models, b, **kw)
    got = ko.knockout_importance(models, b, device="cuda", **kw)
    assert "mixed-architecture ensemble: using the CPU path" in capsys.readouterr().out
    _assert_cpu_numbers(got, ref)


def test_argument_errors():
    b, models = _batch(), _models("h64x2_r4", 1)
    eng = _engine(models, b)
    m, q = ko.scenario_masks([()], 46), ko.macro_scenario_masks([(0,)], M)
    base, mbase = [0.0] * 46, [0.0] * M
    bad = q.copy()
    bad[0, 0] = np.uint32(1 << M)                                    # series M
    with pytest.raises(ValueError, match="macro series outside"):
        eng.eng.knockout_macro(0, m, bad, 1, base, mbase)
    badc = m.copy()
    badc[0, 1] = np.uint32(1 << 14)                                  # column 46
    with pytest.raises(ValueError, match="column outside"):
        eng.eng.knockout_macro(0, badc, q, 1, base, mbase)
    with pytest.raises(ValueError, match="macro_masks"):
        eng.eng.knockout_macro(0, m, np.zeros((1, 2), dtype=np.uint32), 1, base, mbase)
    with pytest.raises(ValueError, match="masks"):
        eng.eng.knockout_macro(0, m, q, 2, base, mbase)
    with pytest.raises(ValueError, match="base"):
        eng.eng.knockout_macro(0, m, q, 1, base[:-1], mbase)
    with pytest.raises(ValueError, match="macro_base"):
        eng.eng.knockout_macro(0, m, q, 1, base, mbase + [0.0])
    with pytest.raises(ValueError, match="no scenarios"):
        eng.eng.knockout_macro(0, m, q, 0, base, mbase)
    with pytest.raises(ValueError, match="split"):
        eng.eng.knockout_macro(1, m, q, 1, base, mbase)              # an unset split
    with pytest.raises(ValueError, match="split"):
        eng.eng.knockout_macro(3, m, q, 1, base, mbase)
    assert not eng.eng.knockout_macro_supported(1)
    with pytest.raises(ValueError, match="outside"):
        ko.knockout_importance(models, b, macro_groups={"g": [M]}, device="cuda")
    # a sharded engine (any hook) is refused before a launch
    eng.eng.set_xs(lambda what, which, st: None)
    with pytest.raises(ValueError, match="single rank"):
        eng.eng.knockout_macro(0, m, q, 1, base, mbase)
    assert not eng.eng.knockout_macro_supported()
    eng.eng.set_xs(None)
    eng.eng.sync()


def test_evaluate_ensemble_end_to_end(shipped_data, capsys):
    import os

    import golden_cases as gc
    from deeplearninginassetpricing_paperreplication_amd.analysis import ensemble as ens
    ckpts = [gc.path(os.path.join("ensemble_ckpt", f"m{seed}")) for seed in (1, 2)]
    plain = ens.evaluate_ensemble(ckpts, shipped_data, device="cuda", verbose=False)
    kw = dict(verbose=False, knockout=True, knockout_macro=True)
    gpu = ens.evaluate_ensemble(ckpts, shipped_data, device="cuda", **kw)
    assert "using the CPU path" not in capsys.readouterr().out
    cpu = ens.evaluate_ensemble(ckpts, shipped_data, device="cpu", **kw)
    for k in plain:
        assert gpu[k] == plain[k], k
    a, c = gpu["knockout"], cpu["knockout"]
    assert a["path"] == "engine" and c["path"] == "cpu" and a["scenarios"] == c["scenarios"]
    assert len(a["scenarios"]) == 1 + 46 + 8 and a["macro_columns"] == c["macro_columns"]
    mk = [k for k, q in enumerate(a["macro_columns"]) if q]
    err = np.abs(a["factor"] - c["factor"]).max() / np.abs(c["factor"]).max()
    print(f"macro end to end: max |dF| / max |F| {err:.3e}, Spearman of d_sharpe over the macro scenarios "
          f"{_spearman(a['d_sharpe'][mk], c['d_sharpe'][mk]):.4f}, baseline Sharpe {a['sharpe'][0]:.4f} / {c['sharpe'][0]:.4f}")
    assert abs(a["sharpe"][0] - plain["test_sharpe"]) <= 1e-5
