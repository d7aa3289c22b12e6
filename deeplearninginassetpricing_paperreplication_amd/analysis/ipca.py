"""Factor benchmarks on the per-period characteristic Gram: IPCA (Kelly, Pruitt and Su) and
Fama-MacBeth cross-sectional regressions.

Both need, per period ``t`` of a split over its valid rows ``i`` (features ``x`` as the engine
stores them: bf16-rounded on the default GPU path, exact with ``precision="fp32"`` and on the CPU),
only second-order sums:

* ``gram[t] = sum_i x_i x_i'`` [F][F], ``n[t]``, ``sum_r[t] = sum R`` and ``sum_rr[t] = sum R^2``
  (``characteristic_gram``; ``Engine.characteristic_gram`` / ``csrc/k_xgram.hip`` on the GPU), and
* ``sum_x[t] = sum_i x_i`` and ``sum_xr[t] = sum_i x_i R_i`` (``benchmarks.managed_portfolios``).

``augment`` joins them: with ``intercept=True`` the characteristics get a constant column,
``x~ = [x, 1]``, ``Gt = [[G, sum_x], [sum_x', n]]``, ``qt = [sum_xr, sum_r]`` and ``Fa = F + 1``;
without it ``Gt = G`` and ``qt = sum_xr``. Everything below is float64 on the host and uses the
periods with ``n_t > 0`` only: every ALS step and every period's regression is an ``Fa x Fa``
problem, the one pass over the rows is the Gram.

IPCA, ``R[t,i] = x~[t,i]' Gamma f[t] + e`` with ``Gamma`` [Fa][K], by alternating least squares
(``ipca_from_sums``):

1. start: ``Gamma`` = the top ``K`` eigenvectors of ``sum_t (q_t / n_t)(q_t / n_t)'``;
2. factors: ``f_t = pinv(Gamma' G_t Gamma) Gamma' q_t`` (``hermitian=True``);
3. loadings: ``[sum_t G_t[a][b] f_t[k] f_t[j]] vec(Gamma) = [sum_t q_t[a] f_t[k]]`` by ``lstsq`` (the
   minimum-norm solution: a constant characteristic next to the intercept does no harm);
4. after every step: ``Gamma' Gamma = I``, ``f' f / T'`` diagonal and descending, every factor mean
   ``>= 0``;
5. stop at ``max |d Gamma| <= tol`` or after ``max_iter`` steps.

``ipca_split_stats`` evaluates given loadings and SDF weights ``b`` on a split from its sums alone:
``f_t``, the SDF factor ``F_t = b' f_t``, the per-period weight vector
``theta_t = Gamma pinv(Gamma' G_t Gamma) b`` (the portfolio ``w = x~ . theta_t`` has
``sum w R = F_t``), ``S2 = theta' G theta``, ``SR = theta' q``,
``SSE_t = sum_rr - 2 f' Gamma' q + f' Gamma' G Gamma f``,
``ev_factors = 1 - sum_t (SSE_t / n_t) / sum_t (sum_rr / n_t)``, ``ev`` by the formula of
``benchmarks.ev_from_sums`` with the SDF weights as loadings, and the Sharpe ratio of ``F_t`` by
``portfolio.sharpe_ddof0`` (over all periods; an empty period has ``F_t = 0``).

``ipca_benchmark`` estimates on train for every ``K`` of ``factors``, sets
``b = pinv(cov_ddof0(f)) mean(f)`` on train, selects ``K`` by ``benchmarks.select`` (``np.argmax`` of
the validation Sharpe) and returns a row shaped like the LS / EN rows.

Fama-MacBeth (``fama_macbeth``): per period with ``n_t > Fa``, ``lambda_t = pinv(Gt_t) qt_t``; the
table holds the mean slope, its t statistic ``mean / (std_ddof1 / sqrt(T'))`` over the used periods,
the mean cross-sectional ``R^2_t = 1 - SSE_t / (sum_rr - sum_r^2 / n)`` (centred with an intercept,
``1 - SSE_t / sum_rr`` without) and the number of periods used.

Out of scope: weighted Grams and value weighting, instrumented alphas (``Gamma_alpha``),
estimation on the GPU, plots, any change to training.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

from . import benchmarks as bm
from .benchmarks import SPLITS, _np
from .portfolio import cross_sectional_r2, sharpe_ddof0


# ---------------------------------------------------------------------------------------------
# The sums

def characteristic_gram_numpy(x, returns, mask) -> Dict:
    """``gram`` float64 [T][F][F], ``n`` int32 [T], ``sum_r``, ``sum_rr`` float64 [T] and ``rows`` of a
    dense split ``x`` [T][N][F], ``returns`` [T][N], ``mask`` [T][N]."""
    x, r, m = _np(x), _np(returns, np.float64), _np(mask).astype(bool)
    T, N, F = x.shape
    g, sr, srr = np.zeros((T, F, F)), np.zeros(T), np.zeros(T)
    for t in range(T):
        idx = np.nonzero(m[t])[0]
        if idx.size:
            xt = x[t, idx].astype(np.float64)
            g[t] = xt.T @ xt
            g[t] = np.triu(g[t]) + np.triu(g[t], 1).T
            sr[t], srr[t] = r[t, idx].sum(), (r[t, idx] * r[t, idx]).sum()
    return {"gram": g, "n": m.sum(axis=1).astype(np.int32), "sum_r": sr, "sum_rr": srr, "rows": int(m.sum())}


def _gram_panel(batches: Sequence[Dict], device: str, precision: str):
    """The device's panel object (``benchmarks._CpuPanel`` / ``_GpuPanel``). The Gram kernel has no
    shape limit, so the GPU panel is used whenever the native extension is there."""
    if str(device).startswith("cuda"):
        from ..ops import native
        if native.load(required=False) is None:
            print("[ipca] native extension not available: using the CPU path")
        else:
            return bm._GpuPanel(batches, precision)
    return bm._CpuPanel(batches)


def characteristic_gram(batch: Dict, device: str = "cpu", precision: str = "bf16") -> Dict:
    """The Gram sums of ``batch`` (``characteristic_gram_numpy``'s keys; ``gpu_ms`` on the GPU)."""
    return _gram_panel([batch], device, precision).gram(0)


def augment(gram: Dict, managed: Dict, intercept: bool = True) -> Dict:
    """``G`` [T][Fa][Fa], ``q`` [T][Fa], ``n`` [T], ``sum_r``, ``sum_rr`` [T] from the two sums of a
    split; ``Fa = F + 1`` with the constant column last when ``intercept``."""
    G, n = np.asarray(gram["gram"], dtype=np.float64), np.asarray(gram["n"])
    sx, sxr = np.asarray(managed["sum_x"], dtype=np.float64), np.asarray(managed["sum_xr"], dtype=np.float64)
    sr, srr = np.asarray(gram["sum_r"], dtype=np.float64), np.asarray(gram["sum_rr"], dtype=np.float64)
    T, F = sx.shape
    if G.shape != (T, F, F) or not np.array_equal(n, np.asarray(managed["n"])):
        raise ValueError("gram and managed sums describe different splits")
    if intercept:
        Gt = np.zeros((T, F + 1, F + 1))
        Gt[:, :F, :F] = G
        Gt[:, :F, F] = sx
        Gt[:, F, :F] = sx
        Gt[:, F, F] = n
        q = np.concatenate([sxr, sr[:, None]], axis=1)
    else:
        Gt, q = G.copy(), sxr.copy()
    return {"G": Gt, "q": q, "n": n.astype(np.int64), "sum_r": sr, "sum_rr": srr, "intercept": bool(intercept)}


def split_sums(panel, s: int, intercept: bool = True) -> Dict:
    """``augment`` of split ``s`` of a panel object, with the GPU time of the two calls."""
    g, m = panel.gram(s), panel.managed(s)
    out = augment(g, m, intercept)
    out["gpu_ms"] = float(g.get("gpu_ms", 0.0)) + float(m.get("gpu_ms", 0.0))
    return out


# ---------------------------------------------------------------------------------------------
# IPCA

def _factors(G: np.ndarray, q: np.ndarray, gamma: np.ndarray):
    """``f_t`` [T][K] and ``pinv(Gamma' G_t Gamma)`` [T][K][K] for every period given."""
    A = np.einsum("ak,tab,bj->tkj", gamma, G, gamma)
    A = 0.5 * (A + A.transpose(0, 2, 1))
    Ainv = np.linalg.pinv(A, hermitian=True) if A.shape[0] else np.zeros_like(A)
    return np.einsum("tkj,tj->tk", Ainv, q @ gamma), Ainv


def _normalise(gamma: np.ndarray, f: np.ndarray):
    """``Gamma' Gamma = I``, ``f' f / T'`` diagonal descending, factor means ``>= 0``; the product
    ``Gamma f_t`` is unchanged where ``Gamma`` has full column rank."""
    Q, R = np.linalg.qr(gamma)
    f = f @ R.T
    w, V = np.linalg.eigh(f.T @ f / max(f.shape[0], 1))
    V = V[:, np.argsort(-w, kind="stable")]
    Q, f = Q @ V, f @ V
    sign = np.where(f.mean(axis=0) < 0, -1.0, 1.0)
    return Q * sign, f * sign


def ipca_from_sums(train: Dict, K: int, gamma=None, tol: float = 1e-8, max_iter: int = 1000) -> Dict:
    """The ALS of the module docstring on the sums of ``augment``. Returns ``gamma`` [Fa][K],
    ``factors`` [T][K] (0 at the empty periods), ``periods`` (the ones used), ``iterations``,
    ``delta`` (the last ``max |d Gamma|``) and ``converged``. ``gamma=`` given skips the estimation:
    the factors of these loadings, ``iterations = 0``."""
    n = np.asarray(train["n"])
    keep = np.nonzero(n > 0)[0]
    G, q = np.asarray(train["G"])[keep], np.asarray(train["q"])[keep]
    T, Fa = np.asarray(train["q"]).shape
    K = int(K)
    if K < 1 or K > Fa:
        raise ValueError(f"K must be in [1, {Fa}]")
    full = np.zeros((T, K))
    if gamma is not None:
        gamma = np.asarray(gamma, dtype=np.float64)
        if gamma.shape != (Fa, K):
            raise ValueError(f"gamma must be [{Fa}][{K}]")
        full[keep] = _factors(G, q, gamma)[0]
        return {"gamma": gamma, "factors": full, "periods": keep, "iterations": 0, "delta": 0.0, "converged": True}
    if keep.size < 1:
        raise ValueError("the train split has no valid rows")
    qb = q / n[keep, None]
    w, V = np.linalg.eigh(qb.T @ qb)
    gamma = V[:, np.argsort(-w, kind="stable")[:K]]
    f = _factors(G, q, gamma)[0]
    gamma, f = _normalise(gamma, f)
    it, delta, conv = 0, np.inf, False
    while it < max_iter:
        it += 1
        f = _factors(G, q, gamma)[0]
        lhs = np.einsum("tab,tk,tj->akbj", G, f, f).reshape(Fa * K, Fa * K)
        rhs = np.einsum("ta,tk->ak", q, f).reshape(Fa * K)
        new = np.linalg.lstsq(lhs, rhs, rcond=None)[0].reshape(Fa, K)
        new, f = _normalise(new, f)
        delta = float(np.abs(new - gamma).max())
        gamma = new
        if delta <= tol:
            conv = True
            break
    full[keep] = f
    return {"gamma": gamma, "factors": full, "periods": keep, "iterations": it, "delta": delta, "converged": conv}


def sdf_weights(factors: np.ndarray) -> np.ndarray:
    """``b = pinv(cov_ddof0(f)) mean(f)`` of a factor sample ``[T'][K]``."""
    f = np.asarray(factors, dtype=np.float64)
    mu = f.mean(axis=0)
    c = (f - mu).T @ (f - mu) / f.shape[0]
    return np.linalg.pinv(c, hermitian=True) @ mu


def ipca_split_stats(sums: Dict, gamma, b) -> Dict:
    """A split's statistics for loadings ``gamma`` [Fa][K] and SDF weights ``b`` [K], from its sums
    alone (no pass over the rows): ``factors`` [T][K], ``factor`` (= ``F_t``) [T], ``theta`` [T][Fa],
    ``s2``, ``sr``, ``sse`` [T], ``ev_factors``, ``ev``, ``sharpe``, ``periods``."""
    gamma, b = np.asarray(gamma, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = np.asarray(sums["n"])
    keep = np.nonzero(n > 0)[0]
    Ga, qa, rr = np.asarray(sums["G"]), np.asarray(sums["q"]), np.asarray(sums["sum_rr"], dtype=np.float64)
    T, Fa = qa.shape
    K = gamma.shape[1]
    G, q = Ga[keep], qa[keep]
    f, Ainv = _factors(G, q, gamma)
    theta = np.einsum("ak,tkj,j->ta", gamma, Ainv, b)
    s2 = np.einsum("ta,tab,tb->t", theta, G, theta)
    sr = np.einsum("ta,ta->t", theta, q)
    gq = q @ gamma
    A = np.einsum("ak,tab,bj->tkj", gamma, G, gamma)
    sse = rr[keep] - 2.0 * np.einsum("tk,tk->t", f, gq) + np.einsum("tk,tkj,tj->t", f, A, f)
    nk = n[keep].astype(np.float64)
    den = (rr[keep] / nk).sum()
    out = {"factors": np.zeros((T, K)), "factor": np.zeros(T), "theta": np.zeros((T, Fa)), "s2": np.zeros(T),
           "sr": np.zeros(T), "sse": np.zeros(T), "periods": keep}
    out["factors"][keep], out["factor"][keep], out["theta"][keep] = f, f @ b, theta
    out["s2"][keep], out["sr"][keep], out["sse"][keep] = s2, sr, sse
    out["ev_factors"] = float(1.0 - (sse / nk).sum() / den) if den > 0 else float("nan")
    out["ev"] = float(bm.ev_from_sums({"s2": out["s2"][:, None], "sr": out["sr"][:, None], "n": n, "sum_rr": rr})[0])
    out["sharpe"] = sharpe_ddof0(out["factor"])
    return out


def _dense_weights(batch: Dict, theta: np.ndarray, intercept: bool) -> np.ndarray:
    """``w[t,i] = x~[t,i] . theta_t`` at the valid entries (0 elsewhere), L1-normalised per period
    where ``sum |w| > 1e-8``: an O(R F) host product from the batch."""
    x = _np(batch["individual_features"], np.float32).astype(np.float64)
    m = _np(batch["mask"]).astype(bool)
    F = x.shape[2]
    w = np.einsum("tnf,tf->tn", x, theta[:, :F])
    if intercept:
        w = w + theta[:, F][:, None]
    w = np.where(m, w, 0.0)
    return bm._normalised(w, np.abs(w).sum(axis=1))


def ipca_benchmark(batches: Dict[str, Dict], factors: Sequence[int] = (1, 2, 3, 4, 5, 6), intercept: bool = True,
                   device: str = "cpu", precision: str = "bf16", gamma=None, tol: float = 1e-8,
                   max_iter: int = 1000) -> Dict:
    """The IPCA row of ``batches`` (``train`` / ``valid`` / ``test`` dicts of ``individual_features``,
    ``returns``, ``mask``): estimation on train for every ``K`` of ``factors``, SDF weights
    ``b = pinv(cov_ddof0(f)) mean(f)`` on train, ``K`` selected by the validation Sharpe.

    Returns ``sharpe`` / ``ev`` / ``ev_factors`` / ``xs_r2`` (dicts by split), ``factor`` and ``weights``
    (by split: [T] and the dense L1-normalised [T][N] float64), ``K``, ``gamma`` [Fa][K], ``b``,
    ``iterations``, ``converged``, ``intercept``, ``device`` and ``candidates`` (per ``K``: ``gamma``,
    ``b``, ``iterations``, ``converged``, ``delta`` and by split ``sharpe``, ``ev``, ``ev_factors``).

    The Gram and the managed sums come from ``device`` (one pass over the rows each); every
    statistic but two follows from them. The dense weights and ``xs_r2``
    (``portfolio.cross_sectional_r2``) of the selected ``K`` are formed on the host from the batch,
    an O(R F) numpy product, as ``benchmarks.linear_benchmarks`` does for its selected rows.

    ``gamma``: loadings [Fa][K] (or a dict ``{K: loadings}``) that skip the estimation, so the two
    devices can be compared on the same loadings; ``factors`` must then name exactly these ``K``."""
    for s in SPLITS:
        if s not in batches:
            raise ValueError(f"batches must hold {SPLITS}")
    bl = [batches[s] for s in SPLITS]
    panel = _gram_panel(bl, device, precision)
    sums = [split_sums(panel, s, intercept) for s in range(3)]
    if gamma is not None and not isinstance(gamma, dict):
        gamma = {int(np.asarray(gamma).shape[1]): gamma}
    Ks = [int(k) for k in factors]
    if not Ks:
        raise ValueError("factors must name at least one K")
    cand: List[Dict] = []
    for K in Ks:
        if gamma is not None and K not in gamma:
            raise ValueError(f"gamma holds no loadings for K = {K}")
        fit = ipca_from_sums(sums[0], K, None if gamma is None else gamma[K], tol, max_iter)
        if fit["periods"].size < 1:
            raise ValueError("the train split has no valid rows")
        b = sdf_weights(fit["factors"][fit["periods"]])
        c = {"K": K, "gamma": fit["gamma"], "b": b, "iterations": fit["iterations"], "converged": fit["converged"],
             "delta": fit["delta"], "stats": [ipca_split_stats(sums[s], fit["gamma"], b) for s in range(3)]}
        for s, name in enumerate(SPLITS):
            c[name] = {k: c["stats"][s][k] for k in ("sharpe", "ev", "ev_factors")}
        cand.append(c)
    best = bm.select([c["valid"]["sharpe"] for c in cand])
    sel = cand[best]
    out = {"K": sel["K"], "gamma": sel["gamma"], "b": sel["b"], "iterations": sel["iterations"],
           "converged": sel["converged"], "intercept": bool(intercept), "index": best,
           "sharpe": {}, "ev": {}, "ev_factors": {}, "xs_r2": {}, "factor": {}, "weights": {}}
    for s, name in enumerate(SPLITS):
        stt = sel["stats"][s]
        w = _dense_weights(bl[s], stt["theta"], intercept)
        out["sharpe"][name], out["ev"][name], out["ev_factors"][name] = stt["sharpe"], stt["ev"], stt["ev_factors"]
        out["factor"][name], out["weights"][name] = stt["factor"], w
        out["xs_r2"][name] = cross_sectional_r2(w, _np(bl[s]["returns"], np.float64), _np(bl[s]["mask"]).astype(bool))
    out["candidates"] = [{k: v for k, v in c.items() if k != "stats"} for c in cand]
    out["device"] = "cuda" if isinstance(panel, bm._GpuPanel) else "cpu"
    if isinstance(panel, bm._GpuPanel):
        out["gpu_ms"] = float(sum(s["gpu_ms"] for s in sums))
    return out


def format_ipca_row(row: Dict) -> str:
    """The IPCA line of the benchmark table (``benchmarks.format_benchmarks``'s columns)."""
    g = lambda d, s: d.get(s, float("nan"))
    return (f"  {'IPCA (K=%d)' % row['K']:14s} {g(row['sharpe'], 'train'):9.4f} {g(row['sharpe'], 'valid'):9.4f} "
            f"{g(row['sharpe'], 'test'):9.4f} {g(row['ev'], 'test'):9.4f} {g(row['xs_r2'], 'test'):11.4f}")


# ---------------------------------------------------------------------------------------------
# Fama-MacBeth

def fama_macbeth(data: Dict, intercept: bool = True, device: str = "cpu", precision: str = "bf16") -> Dict:
    """Cross-sectional regressions of ``R`` on the characteristics, period by period. ``data``: a
    batch (``individual_features``, ``returns``, ``mask``; its sums come from ``device``) or the sums
    of ``augment`` (``intercept`` is then the one they were built with).

    Returns ``slopes`` [T'][Fa] (the constant last), ``mean``, ``tstat`` [Fa] (ddof 1 over the used
    periods; NaN with fewer than two or a zero spread), ``r2`` [T'], ``mean_r2``, ``periods`` (the
    ones with ``n_t > Fa``), ``used`` and ``intercept``."""
    if "G" in data:
        sums = data
        intercept = bool(sums.get("intercept", intercept))
    else:
        sums = split_sums(_gram_panel([data], device, precision), 0, intercept)
    G, q, n = np.asarray(sums["G"]), np.asarray(sums["q"]), np.asarray(sums["n"])
    sr, srr = np.asarray(sums["sum_r"]), np.asarray(sums["sum_rr"])
    Fa = q.shape[1]
    keep = np.nonzero(n > Fa)[0]
    lam = np.einsum("tab,tb->ta", np.linalg.pinv(G[keep], hermitian=True), q[keep]) if keep.size else np.zeros((0, Fa))
    sse = srr[keep] - 2.0 * np.einsum("ta,ta->t", lam, q[keep]) + np.einsum("ta,tab,tb->t", lam, G[keep], lam)
    tot = srr[keep] - (sr[keep] ** 2 / n[keep] if intercept else 0.0)
    r2 = np.where(tot > 0, 1.0 - sse / np.where(tot > 0, tot, 1.0), np.nan)
    Tu = int(keep.size)
    mean = lam.mean(axis=0) if Tu else np.full(Fa, np.nan)
    tstat = np.full(Fa, np.nan)
    if Tu > 1:
        se = lam.std(axis=0, ddof=1) / np.sqrt(Tu)
        tstat = np.divide(mean, se, out=np.full(Fa, np.nan), where=se > 0)
    return {"slopes": lam, "mean": mean, "tstat": tstat, "r2": r2,
            "mean_r2": float(np.nanmean(r2)) if Tu and np.isfinite(r2).any() else float("nan"),
            "periods": keep, "used": Tu, "intercept": bool(intercept)}


def format_fama_macbeth(res: Dict, names: Optional[Sequence[str]] = None) -> List[str]:
    """The printed slope table: one line per characteristic (``names`` or their indices), the
    constant last."""
    Fa = len(res["mean"])
    F = Fa - 1 if res["intercept"] else Fa
    names = [str(v) for v in names] if names is not None else [f"x{j}" for j in range(F)]
    labels = list(names[:F]) + (["const"] if res["intercept"] else [])
    lines = [f"  Fama-MacBeth: {res['used']} periods, mean cross-sectional R2 {res['mean_r2']:.4f}",
             f"  {'':14s} {'slope':>12s} {'t':>9s}"]
    for j, lab in enumerate(labels):
        lines.append(f"  {lab[:14]:14s} {res['mean'][j]:12.5e} {res['tstat'][j]:9.3f}")
    return lines


def fama_macbeth_json(res: Dict, names: Optional[Sequence[str]] = None) -> Dict:
    out = {k: res[k] for k in ("mean", "tstat", "r2", "mean_r2", "periods", "used", "intercept")}
    if names is not None:
        out["names"] = [str(v) for v in names]
    return bm._jsonable(out)
