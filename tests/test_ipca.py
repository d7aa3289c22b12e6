"""The factor benchmarks on the characteristic Gram (``analysis.ipca``) on the CPU: the numpy Gram
against a plain loop, the sums-only SSE against the dense residuals, the ALS on planted panels
(recovery of the loading space, the normalisation, rank-deficient and degenerate periods),
Fama-MacBeth against per-period ``lstsq``, and the evaluator's flags.

The planted panel draws, from ``default_rng(seed)`` in this order: ``x ~ N(0, 1)`` float32 [T][N][F],
``Gamma0 = qr(normal [F][K])``, ``f = normal [T][K] * (0.08, 0.05, 0.03)[:K] + (0.03, 0.01, 0.02)[:K]``,
``r = x Gamma0 f + 0.1 normal`` and ``mask = uniform > 0.2``. A prototype of the ALS converged on
(60, 200, 8, K=2, seed 0) to 1e-8 in 6 iterations with ``|Gamma Gamma' - Gamma0 Gamma0'|_max`` = 0.028,
on (60, 200, 8, 3, seed 1) in 8 with 0.037, on (40, 120, 6, 1, seed 2) and (48, 300, 12, 2, seed 3) in 6;
the noise in ``r`` sets the projector error, so the assertions are ``converged``, at most 50
iterations and a projector error of at most 0.1."""
import json
import os

import numpy as np
import pytest

import golden_cases as gc
from deeplearninginassetpricing_paperreplication_amd.analysis import benchmarks as bm
from deeplearninginassetpricing_paperreplication_amd.analysis import ensemble as ens
from deeplearninginassetpricing_paperreplication_amd.analysis import ipca
from deeplearninginassetpricing_paperreplication_amd.analysis.portfolio import sharpe_ddof0

PLANTED = [(60, 200, 8, 2, 0), (60, 200, 8, 3, 1), (40, 120, 6, 1, 2), (48, 300, 12, 2, 3)]
_CACHE = {}


def planted(T, N, F, K, seed):
    key = (T, N, F, K, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        x = rng.standard_normal((T, N, F)).astype(np.float32)
        g0 = np.linalg.qr(rng.standard_normal((F, K)))[0]
        f = rng.standard_normal((T, K)) * np.array((0.08, 0.05, 0.03))[:K] + np.array((0.03, 0.01, 0.02))[:K]
        r = np.einsum("tnf,fk,tk->tn", x.astype(np.float64), g0, f) + 0.1 * rng.standard_normal((T, N))
        mask = rng.uniform(size=(T, N)) > 0.2
        _CACHE[key] = (x, r.astype(np.float32), mask, g0)
    return _CACHE[key]


def _sums(x, r, m, intercept=True):
    return ipca.augment(ipca.characteristic_gram_numpy(x, r, m), bm.managed_portfolios_numpy(x, r, m), intercept)


def _xa(x, intercept):
    x = x.astype(np.float64)
    return np.concatenate([x, np.ones(x.shape[:2] + (1,))], axis=2) if intercept else x


def test_gram_equals_a_plain_loop():
    x, r, m = planted(7, 23, 5, 1, 11)[:3]
    m = m.copy()
    m[3] = False
    got = ipca.characteristic_gram_numpy(x, r, m)
    T, N, F = x.shape
    for t in range(T):
        g, sr, srr = np.zeros((F, F)), 0.0, 0.0
        for i in range(N):
            if m[t, i]:
                xi = x[t, i].astype(np.float64)
                g += np.outer(xi, xi)
                sr += float(r[t, i])
                srr += float(r[t, i]) ** 2
        np.testing.assert_allclose(got["gram"][t], g, rtol=0, atol=1e-12)
        np.testing.assert_allclose([got["sum_r"][t], got["sum_rr"][t]], [sr, srr], rtol=0, atol=1e-13)
        assert (got["gram"][t] == got["gram"][t].T).all()
    assert got["gram"].dtype == np.float64 and got["gram"].shape == (T, F, F)
    assert got["n"].dtype == np.int32 and (got["n"] == m.sum(1)).all() and got["rows"] == int(m.sum())
    assert got["n"][3] == 0 and (got["gram"][3] == 0).all()
    api = ipca.characteristic_gram({"individual_features": x, "returns": r, "mask": m})
    assert api["gram"].tobytes() == got["gram"].tobytes()


@pytest.mark.parametrize("intercept", [True, False])
def test_augment(intercept):
    x, r, m = planted(7, 23, 5, 1, 11)[:3]
    s = _sums(x, r, m, intercept)
    xa = _xa(x, intercept)
    for t in range(x.shape[0]):
        xt, rt = xa[t, m[t]], r[t, m[t]].astype(np.float64)
        np.testing.assert_allclose(s["G"][t], xt.T @ xt, rtol=0, atol=1e-11)
        np.testing.assert_allclose(s["q"][t], xt.T @ rt, rtol=0, atol=1e-12)
    assert s["G"].shape[1] == 5 + int(intercept)
    bad = bm.managed_portfolios_numpy(x, r, ~m)
    with pytest.raises(ValueError):
        ipca.augment(ipca.characteristic_gram_numpy(x, r, m), bad)


def test_sse_from_the_sums_equals_the_dense_residuals():
    x, r, m, _ = planted(*PLANTED[0])
    s = _sums(x, r, m)
    rng = np.random.default_rng(4)
    gamma = np.linalg.qr(rng.standard_normal((9, 2)))[0]
    b = np.array([1.5, -0.5])
    st = ipca.ipca_split_stats(s, gamma, b)
    xa = _xa(x, True)
    sse, sr, s2 = np.zeros(60), np.zeros(60), np.zeros(60)
    for t in range(60):
        xt, rt = xa[t, m[t]], r[t, m[t]].astype(np.float64)
        z = xt @ gamma
        f = np.linalg.lstsq(z, rt, rcond=None)[0]
        np.testing.assert_allclose(st["factors"][t], f, rtol=1e-9, atol=1e-12)
        e = rt - z @ f
        sse[t] = e @ e
        w = xt @ st["theta"][t]
        sr[t], s2[t] = w @ rt, w @ w
    np.testing.assert_allclose(st["sse"], sse, rtol=1e-12)
    np.testing.assert_allclose(st["sr"], sr, rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(st["s2"], s2, rtol=1e-10)
    np.testing.assert_allclose(st["factor"], st["factors"] @ b, rtol=1e-13)
    np.testing.assert_allclose(st["sr"], st["factor"], rtol=1e-9, atol=1e-13)      # the portfolio's return is F_t
    n = m.sum(1)
    rr = np.where(m, r, 0).astype(np.float64)
    den = ((rr * rr).sum(1) / n).sum()
    assert st["ev_factors"] == pytest.approx(1 - (sse / n).sum() / den, rel=1e-12)
    assert st["ev"] == pytest.approx(1 - (((rr * rr).sum(1) - sr * sr / s2) / n).sum() / den, rel=1e-10)
    assert st["sharpe"] == sharpe_ddof0(st["factor"])


def _check_normalised(fit):
    g, f = fit["gamma"], fit["factors"][fit["periods"]]
    K = g.shape[1]
    np.testing.assert_allclose(g.T @ g, np.eye(K), atol=1e-12)
    c = f.T @ f / f.shape[0]
    d = np.diag(c)
    assert np.abs(c - np.diag(d)).max() <= 1e-12 * d.max()
    assert (np.diff(d) <= 0).all()
    assert (f.mean(0) >= 0).all()


@pytest.mark.parametrize("intercept", [False, True])
@pytest.mark.parametrize("case", PLANTED)
def test_planted_loadings_are_recovered(case, intercept):
    T, N, F, K, seed = case
    x, r, m, g0 = planted(*case)
    fit = ipca.ipca_from_sums(_sums(x, r, m, intercept), K)
    g = fit["gamma"][:F]
    err = np.abs(g @ g.T - g0 @ g0.T).max()
    print(f"planted {case} intercept={intercept}: {fit['iterations']} iterations, delta {fit['delta']:.2e}, "
          f"projector error {err:.4f}")
    assert fit["converged"] and fit["iterations"] <= 50 and fit["delta"] <= 1e-8
    assert err <= 0.1
    _check_normalised(fit)
    assert fit["factors"].shape == (T, K) and fit["periods"].tolist() == list(range(T))


def test_constant_column_with_the_intercept_still_converges():
    """``Gt`` is rank-deficient (two identical columns up to scale): pinv and the minimum-norm lstsq."""
    x, r, m, g0 = planted(*PLANTED[0])
    x = x.copy()
    x[:, :, 3] = 0.5
    r = (np.einsum("tnf,fk,tk->tn", x.astype(np.float64), g0,
                   np.random.default_rng(9).standard_normal((60, 2)) * 0.05 + 0.02)
         + 0.1 * np.random.default_rng(10).standard_normal(r.shape)).astype(np.float32)
    s = _sums(x, r, m, True)
    assert np.linalg.matrix_rank(s["G"][0]) == 8
    fit = ipca.ipca_from_sums(s, 2)
    assert fit["converged"] and fit["iterations"] <= 50 and np.isfinite(fit["gamma"]).all()
    _check_normalised(fit)
    st = ipca.ipca_split_stats(s, fit["gamma"], ipca.sdf_weights(fit["factors"]))
    assert np.isfinite(st["sse"]).all() and (st["sse"] >= 0).all() and 0 < st["ev_factors"] < 1


def test_short_and_empty_periods_are_handled():
    x, r, m, g0 = planted(*PLANTED[1])
    m = m.copy()
    m[4] = False                                        # empty
    m[9] = False
    m[9, :2] = True                                     # n_t = 2 < K = 3
    s = _sums(x, r, m, False)
    fit = ipca.ipca_from_sums(s, 3)
    assert fit["converged"] and fit["iterations"] <= 50
    assert 4 not in fit["periods"] and 9 in fit["periods"] and (fit["factors"][4] == 0).all()
    assert np.isfinite(fit["factors"]).all()
    g = fit["gamma"]
    assert np.abs(g @ g.T - g0 @ g0.T).max() <= 0.1
    st = ipca.ipca_split_stats(s, g, ipca.sdf_weights(fit["factors"][fit["periods"]]))
    assert st["factor"][4] == 0 and np.isfinite(st["factor"]).all() and np.isfinite(st["ev"])
    assert abs(st["sse"][9]) <= 1e-12 * s["sum_rr"][9] + 1e-15      # two rows, three factors: an exact fit
    with pytest.raises(ValueError):
        ipca.ipca_from_sums(s, 0)
    with pytest.raises(ValueError):
        ipca.ipca_from_sums(s, 3, gamma=np.zeros((8, 2)))
    empty = _sums(x, r, np.zeros_like(m), False)
    with pytest.raises(ValueError):
        ipca.ipca_from_sums(empty, 1)


def test_given_loadings_skip_the_estimation():
    x, r, m, g0 = planted(*PLANTED[0])
    s = _sums(x, r, m, False)
    fit = ipca.ipca_from_sums(s, 2, gamma=g0)
    assert fit["iterations"] == 0 and fit["converged"] and fit["gamma"] is not None
    np.testing.assert_array_equal(fit["gamma"], g0)
    for t in (0, 17):
        z = x[t, m[t]].astype(np.float64) @ g0
        np.testing.assert_allclose(fit["factors"][t], np.linalg.lstsq(z, r[t, m[t]].astype(np.float64), rcond=None)[0],
                                   rtol=1e-9)


def _batches(case, cuts):
    x, r, m, g0 = planted(*case)
    out, a = {}, 0
    for name, k in zip(bm.SPLITS, cuts):
        out[name] = {"individual_features": x[a:a + k], "returns": r[a:a + k], "mask": m[a:a + k]}
        a += k
    return out


def test_benchmark_row():
    batches = _batches(PLANTED[0], (36, 12, 12))
    row = ipca.ipca_benchmark(batches, factors=(1, 2, 3))
    assert row["device"] == "cpu" and row["K"] in (1, 2, 3) and row["gamma"].shape == (9, row["K"])
    assert len(row["candidates"]) == 3 and all(c["converged"] for c in row["candidates"])
    vs = [c["valid"]["sharpe"] for c in row["candidates"]]
    assert row["index"] == int(np.argmax(vs)) and row["sharpe"]["valid"] == max(vs)
    for s in bm.SPLITS:
        b = batches[s]
        w, m = row["weights"][s], b["mask"]
        assert w.shape == m.shape and (w[~m] == 0).all()
        np.testing.assert_allclose(np.abs(w).sum(1), 1.0, atol=1e-12)
        assert row["factor"][s].shape == (m.shape[0],)
        assert row["sharpe"][s] == sharpe_ddof0(row["factor"][s])
        # the dense weights are the normalised x~ . theta_t: their return is F_t / sum |w|
        st = ipca.ipca_split_stats(ipca.split_sums(bm._CpuPanel([b]), 0), row["gamma"], row["b"])
        raw = np.where(m, np.einsum("tnf,tf->tn", _xa(b["individual_features"], True), st["theta"]), 0.0)
        np.testing.assert_allclose((raw * b["returns"]).sum(1), st["factor"], rtol=1e-8, atol=1e-12)
        np.testing.assert_allclose(w, raw / np.abs(raw).sum(1, keepdims=True), rtol=1e-12, atol=1e-15)
        assert np.isfinite(row["xs_r2"][s]) and 0 < row["ev_factors"][s] < 1
    two = ipca.ipca_benchmark(batches, factors=(2,), gamma=row["candidates"][1]["gamma"])
    assert two["iterations"] == 0 and two["K"] == 2
    assert two["sharpe"]["test"] == pytest.approx(row["candidates"][1]["test"]["sharpe"], rel=1e-9)
    line = ipca.format_ipca_row(row)
    assert line.split()[:2] == ["IPCA", f"(K={row['K']})"]
    json.dumps(bm._jsonable({k: v for k, v in row.items() if k != "weights"}))


@pytest.mark.parametrize("intercept", [True, False])
def test_fama_macbeth_matches_lstsq(intercept):
    x, r, m, _ = planted(*PLANTED[3])
    m = m.copy()
    m[5] = False
    m[7] = False
    m[7, :13 if intercept else 12] = True               # n_t = Fa: not used (needs n_t > Fa)
    fm = ipca.fama_macbeth({"individual_features": x, "returns": r, "mask": m}, intercept=intercept)
    used = [t for t in range(48) if t not in (5, 7)]
    assert fm["periods"].tolist() == used and fm["used"] == 46
    xa = _xa(x, intercept)
    lam, r2 = [], []
    for t in used:
        xt, rt = xa[t, m[t]], r[t, m[t]].astype(np.float64)
        l = np.linalg.lstsq(xt, rt, rcond=None)[0]
        e = rt - xt @ l
        lam.append(l)
        r2.append(1 - e @ e / (((rt - rt.mean()) ** 2).sum() if intercept else rt @ rt))
    lam = np.array(lam)
    np.testing.assert_allclose(fm["slopes"], lam, rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(fm["mean"], lam.mean(0), rtol=1e-8, atol=1e-13)
    np.testing.assert_allclose(fm["tstat"], lam.mean(0) / (lam.std(0, ddof=1) / np.sqrt(46)), rtol=1e-7)
    np.testing.assert_allclose(fm["r2"], r2, rtol=1e-8)
    assert fm["mean_r2"] == pytest.approx(np.mean(r2), rel=1e-8)
    same = ipca.fama_macbeth(_sums(x, r, m, intercept))
    assert same["slopes"].tobytes() == fm["slopes"].tobytes() and same["intercept"] == intercept
    lines = ipca.format_fama_macbeth(fm)
    assert len(lines) == 2 + 12 + int(intercept) and (lines[-1].split()[0] == "const") == intercept


def _ckpts():
    return [gc.path(os.path.join("ensemble_ckpt", f"m{seed}")) for seed in (1, 2)]


def test_cli_flags_add_the_ipca_row_and_the_slope_table(shipped_data, tmp_path, capsys):
    common = ["--data_dir", shipped_data, "--checkpoint_dirs", *_ckpts(), "--benchmarks", "--benchmark_grid", "4x1"]
    base = ens.main(common + ["--benchmarks_out", str(tmp_path / "base.json")])
    base_text = capsys.readouterr().out
    jb, jf = tmp_path / "bench.json", tmp_path / "fm.json"
    got = ens.main(common + ["--benchmark_ipca", "--ipca_factors", "1", "2", "--fama_macbeth", "--sort_split", "valid",
                             "--benchmarks_out", str(jb), "--fm_out", str(jf)])
    text = capsys.readouterr().out
    assert "IPCA" not in base_text and "FAMA-MACBETH" not in base_text
    tab = text[text.index("BENCHMARK SDFS"):].splitlines()
    rows = [ln.split()[0] for ln in tab if ln.startswith("  ") and ln.split() and ln.split()[0] in ("LS", "EN", "IPCA", "GAN")]
    assert rows == ["LS", "EN", "IPCA", "GAN"]
    assert "FAMA-MACBETH REGRESSIONS (valid split)" in text
    assert set(got) == set(base) | {"fama_macbeth"} and set(got["benchmarks"]) == set(base["benchmarks"]) | {"ipca"}
    row = got["benchmarks"]["ipca"]
    assert row["K"] in (1, 2) and row["gamma"].shape == (47, row["K"]) and row["device"] == "cpu"
    d, d0 = json.loads(jb.read_text()), json.loads((tmp_path / "base.json").read_text())
    assert set(d) == set(d0) | {"IPCA"} and "weights" not in d["IPCA"]
    for k in d0:
        assert d[k] == d0[k]
    assert d["IPCA"]["K"] == row["K"] and set(d["IPCA"]["sharpe"]) == set(bm.SPLITS)
    fm = json.loads(jf.read_text())
    assert len(fm["mean"]) == 47 and len(fm["tstat"]) == 47 and fm["used"] == got["fama_macbeth"]["used"]
    with pytest.raises(SystemExit):
        ens.main(common[:4] + ["--benchmark_ipca"])
