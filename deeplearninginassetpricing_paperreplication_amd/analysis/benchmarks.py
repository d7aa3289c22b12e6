"""Linear (LS) and elastic-net (EN) benchmark SDFs: the rows the paper's main table reports next to
the GAN. Both are mean-variance weights that are linear in the characteristics, built on the
characteristic-managed portfolios.

Definitions. For a split with valid rows ``(t, i)``, features ``x`` as the engine stores them
(bf16-rounded on the default GPU path, exact with ``precision="fp32"`` and on the CPU), returns
``R`` and ``n_t`` valid stocks in period ``t``:

* Managed sums: ``sum_x[t][f] = sum_i x``, ``sum_xr[t][f] = sum_i x R``, ``n[t]``, and the managed
  portfolios ``F~[t] = sum_xr[t] / n_t`` for the periods with ``n_t > 0`` (empty periods are
  dropped from estimation).
* Linear portfolios for candidates ``Theta [K][F]`` and a centre ``c [T][K]`` (float32, 0 when
  absent): ``w[t,i,k] = x[t,i,:] . Theta[k]``, ``v = w - c[t][k]`` and, per ``(t, k)`` over the valid
  rows of the period, ``S1 = sum w``, ``SA = sum |v|``, ``S2 = sum v^2``, ``SR = sum v R``; per
  ``t``: ``n``, ``sum_r = sum R`` and ``sum_rr = sum R^2``.
* ``center="mean"`` (default, mirrors the models' ``zero_mean_normalize``):
  ``c[t][k] = float32((sum_x[t] / n_t) . Theta[k])`` from the managed sums, 0 for an empty period;
  ``center="none"``: ``c = 0``.
* Factor (the rule of ``portfolio.renormalize``): ``F_t^k = SR / SA`` if ``SA > 1e-8`` else ``SR``,
  over all ``T`` periods. The sign is the natural one, ``+v.R`` (the GAN's factor is ``-w.R``).
  Sharpe is ``portfolio.sharpe_ddof0(F^k)``.
* ``EV^k = 1 - sum_t[(sum_rr - SR^2 / S2) / max(n, 1)] / sum_t[sum_rr / max(n, 1)]``, the
  ``SR^2 / S2`` term only where ``S2 > 1e-12``: ``portfolio.explained_variation`` with loadings ``v``.

Estimation (host, float64; a 46 x 46 problem) on the train split's ``F~ [T'][F]`` with
``A = F~'F~ / T'`` and ``b = mean_t F~``:

* LS: the minimum-norm solution of ``min |1 - F~ theta|^2`` (``lstsq``; a constant column, i.e. a
  rank-deficient ``F~``, does not break it).
* EN: ``theta(l1, l2) = argmin 1/2 th'A th - b'th + 1/2 l2 |th|^2 + l1 |th|_1`` by cyclic coordinate
  descent, ``th_j = soft(b_j - sum_{m != j} A_jm th_m, l1) / (A_jj + l2)``, warm-started along
  descending ``l1``, stopped at ``max |d th| <= 1e-10 max(1, max |th|)`` or after 10000 sweeps (the
  sweeps used are reported). Default grid: ``l1 = max|b| 10^(-linspace(0, 3, 16))``,
  ``l2 = (trace A / F) {0, 1e-3, 1e-2, 1e-1}``, candidates ordered ``l2``-major (64: one launch).
  Selection: ``np.argmax`` of the validation Sharpe of the normalised factor (first index on ties).

``device="cpu"`` evaluates the definitions with numpy (the oracle). ``device="cuda"`` runs
``Engine.managed_portfolios`` / ``Engine.linear_portfolios`` (``csrc/k_linport.hip``) on the panel
the engine holds in HBM; the kernels read the panel only, so no checkpoint is needed (the engine is
built from a default spec) and the wide layer-0 path is covered. The kernel forms ``w`` in fp32
(exact products, fp32 accumulation on the fp32-input MFMA) and ``v = float32(w - c)``; its sums are
the fp64 sums of exactly the ``v`` it writes (``S1 = sum (v + c)``).

The FFN return-prediction benchmark and the beta network live in ``analysis.prediction``, IPCA and
Fama-MacBeth (on the per-period characteristic Gram, ``gram`` of the panel objects) in ``analysis.ipca``. Out of
scope here: estimation on the GPU, value weighting, plots.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .portfolio import cross_sectional_r2, sharpe_ddof0

MAX_K = 64
SPLITS = ("train", "valid", "test")


def _np(a, dtype=None) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a) if dtype is None else np.asarray(a, dtype=dtype)


def _thetas(thetas, F: int) -> np.ndarray:
    th = np.atleast_2d(np.asarray(thetas, dtype=np.float32))
    if th.ndim != 2 or th.shape[1] != F or th.shape[0] < 1:
        raise ValueError(f"thetas must be [K][{F}]")
    return np.ascontiguousarray(th)


# ---------------------------------------------------------------------------------------------
# The definitions in numpy

def managed_portfolios_numpy(x, returns, mask) -> Dict:
    """``sum_x``, ``sum_xr`` float64 [T][F], ``n`` int32 [T] and ``rows`` of a dense split ``x``
    [T][N][F], ``returns`` [T][N], ``mask`` [T][N]."""
    x, r, m = _np(x), _np(returns, np.float64), _np(mask).astype(bool)
    T, N, F = x.shape
    sx, sxr = np.zeros((T, F)), np.zeros((T, F))
    for t in range(T):
        idx = np.nonzero(m[t])[0]
        if idx.size:
            xt = x[t, idx].astype(np.float64)
            sx[t] = xt.sum(axis=0)
            sxr[t] = (xt * r[t, idx, None]).sum(axis=0)
    return {"sum_x": sx, "sum_xr": sxr, "n": m.sum(axis=1).astype(np.int32), "rows": int(m.sum())}


def linear_sums_numpy(x, returns, mask, thetas, center=None, return_weights: bool = False) -> Dict:
    """The per-period sums of the linear portfolios in float64: ``s1``, ``sa``, ``s2``, ``sr`` [T][K],
    ``n`` int32 [T], ``sum_r``, ``sum_rr`` [T], ``rows``; with ``return_weights`` also ``v`` float64
    [K][T][N] (0 at the invalid entries). ``center``: [T][K] or None."""
    x, r, m = _np(x), _np(returns, np.float64), _np(mask).astype(bool)
    T, N, F = x.shape
    th = _thetas(thetas, F).astype(np.float64)
    K = th.shape[0]
    c = np.zeros((T, K)) if center is None else np.asarray(center, dtype=np.float32).astype(np.float64)
    if c.shape != (T, K):
        raise ValueError(f"center must be [{T}][{K}]")
    out = {k: np.zeros((T, K)) for k in ("s1", "sa", "s2", "sr")}
    sum_r, sum_rr = np.zeros(T), np.zeros(T)
    v_out = np.zeros((K, T, N)) if return_weights else None
    for t in range(T):
        idx = np.nonzero(m[t])[0]
        if not idx.size:
            continue
        w = x[t, idx].astype(np.float64) @ th.T                  # [n][K]
        v = w - c[t][None, :]
        rt = r[t, idx]
        out["s1"][t] = w.sum(axis=0)
        out["sa"][t] = np.abs(v).sum(axis=0)
        out["s2"][t] = (v * v).sum(axis=0)
        out["sr"][t] = (v * rt[:, None]).sum(axis=0)
        sum_r[t], sum_rr[t] = rt.sum(), (rt * rt).sum()
        if return_weights:
            v_out[:, t, idx] = v.T
    out.update(n=m.sum(axis=1).astype(np.int32), sum_r=sum_r, sum_rr=sum_rr, rows=int(m.sum()))
    if return_weights:
        out["v"] = v_out
    return out


def center_from_managed(managed: Dict, thetas, center: str = "mean") -> Optional[np.ndarray]:
    """``c [T][K]`` float32 of the ``center`` option from the managed sums (None for ``"none"``)."""
    if center == "none":
        return None
    if center != "mean":
        raise ValueError("center must be 'mean' or 'none'")
    n = np.asarray(managed["n"]).astype(np.float64)
    th = _thetas(thetas, managed["sum_x"].shape[1]).astype(np.float64)
    mx = np.asarray(managed["sum_x"]) / np.maximum(n, 1.0)[:, None]
    return np.where(n[:, None] > 0, mx @ th.T, 0.0).astype(np.float32)


def managed_factors(managed: Dict) -> Tuple[np.ndarray, np.ndarray]:
    """``F~ [T'][F]`` over the non-empty periods, and their indices."""
    n = np.asarray(managed["n"])
    keep = np.nonzero(n > 0)[0]
    return np.asarray(managed["sum_xr"])[keep] / n[keep, None].astype(np.float64), keep


def factors_from_sums(sums: Dict) -> np.ndarray:
    """``F [T][K]``: ``SR / SA`` where ``SA > 1e-8``, else ``SR``."""
    sa, sr = np.asarray(sums["sa"]), np.asarray(sums["sr"])
    ok = sa > 1e-8
    return np.where(ok, np.divide(sr, sa, out=np.zeros_like(sr), where=ok), sr)


def sharpes_from_sums(sums: Dict) -> np.ndarray:
    f = factors_from_sums(sums)
    return np.array([sharpe_ddof0(f[:, k]) for k in range(f.shape[1])])


def ev_from_sums(sums: Dict) -> np.ndarray:
    """``EV [K]`` from the sums (NaN when the split has no return variation)."""
    s2, sr = np.asarray(sums["s2"]), np.asarray(sums["sr"])
    n = np.maximum(np.asarray(sums["n"]).astype(np.float64), 1.0)
    rr = np.asarray(sums["sum_rr"])
    ok = s2 > 1e-12
    proj = np.divide(sr * sr, s2, out=np.zeros_like(sr), where=ok)
    den = (rr / n).sum()
    num = ((rr[:, None] - proj) / n[:, None]).sum(axis=0)
    return 1.0 - num / den if den > 0 else np.full(s2.shape[1], np.nan)


# ---------------------------------------------------------------------------------------------
# Estimation (host, float64)

def fit_ls(Ft: np.ndarray) -> np.ndarray:
    """Minimum-norm solution of ``min |1 - F~ theta|^2``."""
    Ft = np.asarray(Ft, dtype=np.float64)
    return np.linalg.lstsq(Ft, np.ones(Ft.shape[0]), rcond=None)[0]


def en_moments(Ft: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    Ft = np.asarray(Ft, dtype=np.float64)
    return Ft.T @ Ft / Ft.shape[0], Ft.mean(axis=0)


EN_TOL = 1e-10
EN_MAX_SWEEPS = 10000


def en_path(A: np.ndarray, b: np.ndarray, l1s: Sequence[float], l2: float,
            theta0: Optional[np.ndarray] = None, max_sweeps: int = EN_MAX_SWEEPS) -> Tuple[np.ndarray, List[int]]:
    """Elastic-net solutions [len(l1s)][F] along ``l1s`` in the given order (descending for the
    warm start to help), each started from the previous one (the first from ``theta0`` or 0), and
    the sweeps each point used."""
    A, b = np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64)
    F = b.shape[0]
    th = np.zeros(F) if theta0 is None else np.array(theta0, dtype=np.float64)
    diag = np.diag(A) + float(l2)
    out, used = [], []
    for l1 in l1s:
        l1 = float(l1)
        g = A @ th                                       # kept current: g = A th
        sweeps = 0
        while sweeps < max_sweeps:
            sweeps += 1
            step = 0.0
            for j in range(F):
                rho = b[j] - (g[j] - A[j, j] * th[j])
                new = np.sign(rho) * max(abs(rho) - l1, 0.0) / diag[j] if diag[j] > 0 else 0.0
                d = new - th[j]
                if d != 0.0:
                    g += A[:, j] * d
                    th[j] = new
                    step = max(step, abs(d))
            if step <= EN_TOL * max(1.0, float(np.abs(th).max())):
                break
        out.append(th.copy())
        used.append(sweeps)
    return np.array(out), used


def en_grid(A: np.ndarray, b: np.ndarray, grid=(16, 4)) -> Tuple[np.ndarray, np.ndarray]:
    """The default penalties: ``n1`` values of ``l1`` (descending) and ``n2 <= 4`` of ``l2``."""
    n1, n2 = int(grid[0]), int(grid[1])
    if n1 < 1 or n2 < 1 or n2 > 4:
        raise ValueError("grid must be (n1 >= 1, 1 <= n2 <= 4)")
    l1 = np.abs(b).max() * 10.0 ** (-np.linspace(0.0, 3.0, n1))
    l2 = (np.trace(A) / A.shape[0]) * np.array([0.0, 1e-3, 1e-2, 1e-1])[:n2]
    return l1, l2


def parse_grid(spec) -> Tuple[int, int]:
    """CLI form of ``grid``: ``"16x4"`` (or a pair)."""
    if isinstance(spec, str):
        ab = spec.lower().split("x")
        try:
            spec = (int(ab[0]), int(ab[1])) if len(ab) == 2 else None
        except ValueError:
            spec = None
        if spec is None:
            raise ValueError("benchmark_grid: expected N1xN2")
    n1, n2 = int(spec[0]), int(spec[1])
    if n1 < 1 or n2 < 1 or n2 > 4:
        raise ValueError("benchmark_grid: N1 >= 1 and 1 <= N2 <= 4")
    return n1, n2


def select(valid_sharpes) -> int:
    """Index of the candidate with the largest validation Sharpe (the first on ties)."""
    return int(np.argmax(np.asarray(valid_sharpes)))


# ---------------------------------------------------------------------------------------------
# The two devices behind one interface: managed(split) and sums(split, thetas, center, weights)

class _CpuPanel:
    def __init__(self, batches: Sequence[Dict]):
        self.b = [{"x": _np(b["individual_features"], np.float32), "r": _np(b["returns"], np.float32),
                   "m": _np(b["mask"]).astype(bool)} for b in batches]

    def managed(self, s: int) -> Dict:
        b = self.b[s]
        return managed_portfolios_numpy(b["x"], b["r"], b["m"])

    def gram(self, s: int) -> Dict:
        from .ipca import characteristic_gram_numpy
        b = self.b[s]
        return characteristic_gram_numpy(b["x"], b["r"], b["m"])

    def sums(self, s: int, th: np.ndarray, c, weights: bool) -> Dict:
        b = self.b[s]
        return linear_sums_numpy(b["x"], b["r"], b["m"], th, c, weights)


def default_spec(F: int, M: int):
    """The engine shape the GPU path uses when no model is given (the kernels read the panel only)."""
    from ..config import ModelSpec, default_cli_config
    return ModelSpec.from_config(default_cli_config(M, F, hidden_dim=[64, 64], rnn_dim=[4], dropout=0.05,
                                                    use_lstm=M > 0))


class _GpuPanel:
    def __init__(self, batches: Sequence[Dict], precision: str, spec=None):
        from ..engine.runner import GANEngine
        b0 = batches[0]
        F = int(b0["individual_features"].shape[2])
        mac = b0.get("macro_features")
        M = 0 if mac is None else int(mac.shape[1])
        self.eng = GANEngine(spec or default_spec(F, M), 1, max_epochs=4, precision=precision)
        self.eng.set_data(*batches)
        self.shapes = [tuple(b["mask"].shape) for b in batches]
        self.dev = torch.device("cuda", torch.cuda.current_device())

    def supported(self) -> bool:
        return bool(self.eng.eng.linear_supported())

    def managed(self, s: int) -> Dict:
        r = self.eng.eng.managed_portfolios(s)
        return {"sum_x": np.asarray(r["sum_x"]), "sum_xr": np.asarray(r["sum_xr"]), "n": np.asarray(r["n"]),
                "rows": int(r["rows"]), "gpu_ms": float(r["gpu_ms"])}

    def gram(self, s: int) -> Dict:
        r = self.eng.eng.characteristic_gram(s)
        return {"gram": np.asarray(r["gram"]), "n": np.asarray(r["n"]), "sum_r": np.asarray(r["sum_r"]),
                "sum_rr": np.asarray(r["sum_rr"]), "rows": int(r["rows"]), "gpu_ms": float(r["gpu_ms"])}

    def sums(self, s: int, th: np.ndarray, c, weights: bool) -> Dict:
        T, N = self.shapes[s]
        K = th.shape[0]
        w = torch.zeros((K, T, N), dtype=torch.float32, device=self.dev) if weights else None
        torch.cuda.synchronize(self.dev)
        try:
            r = self.eng.eng.linear_portfolios(s, th, c, w.data_ptr() if weights else 0)
        finally:
            self.eng.eng.sync()
        out = {k: np.asarray(r[k]) for k in ("s1", "sa", "s2", "sr", "n", "sum_r", "sum_rr")}
        out.update(rows=int(r["rows"]), gpu_ms=float(r["gpu_ms"]))
        if weights:
            out["v"] = w.cpu().numpy().astype(np.float64)
        return out


def _panel(batches: Sequence[Dict], device: str, precision: str, tag: str):
    """The device's panel object; the CPU one (with a printed note) where the GPU path is not
    available."""
    if str(device).startswith("cuda"):
        from ..ops import native
        if native.load(required=False) is None:
            print(f"[{tag}] native extension not available: using the CPU path")
        else:
            p = _GpuPanel(batches, precision)
            if p.supported():
                return p
            print(f"[{tag}] linear_portfolios: not available for this shape: using the CPU path")
    return _CpuPanel(batches)


def _chunked_sums(panel, s: int, th: np.ndarray, c, weights: bool = False) -> Dict:
    """``panel.sums`` over chunks of at most MAX_K candidates, concatenated."""
    parts = [panel.sums(s, th[k:k + MAX_K], None if c is None else np.ascontiguousarray(c[:, k:k + MAX_K]), weights)
             for k in range(0, th.shape[0], MAX_K)]
    out = dict(parts[0])
    for k in ("s1", "sa", "s2", "sr"):
        out[k] = np.concatenate([p[k] for p in parts], axis=1)
    if weights:
        out["v"] = np.concatenate([p["v"] for p in parts], axis=0)
    if "gpu_ms" in out:
        out["gpu_ms"] = float(sum(p["gpu_ms"] for p in parts))
    return out


def managed_portfolios(batch: Dict, device: str = "cpu", precision: str = "bf16") -> Dict:
    """The managed sums of ``batch`` (``managed_portfolios_numpy``'s keys; ``gpu_ms`` on the GPU)."""
    return _panel([batch], device, precision, "benchmarks").managed(0)


def linear_sums(batch: Dict, thetas, device: str = "cpu", center: str = "mean", precision: str = "bf16",
                return_weights: bool = False) -> Dict:
    """The sums of ``linear_sums_numpy`` for ``thetas [K][F]`` (any ``K``: chunks of 64) on
    ``device``, with the ``center`` option evaluated from the same device's managed sums; the
    centre used is returned as ``center`` ([T][K] float32 or None)."""
    panel = _panel([batch], device, precision, "benchmarks")
    th = _thetas(thetas, int(batch["individual_features"].shape[2]))
    c = center_from_managed(panel.managed(0), th, center)
    out = _chunked_sums(panel, 0, th, c, return_weights)
    out["center"] = c
    return out


def _normalised(v: np.ndarray, sa: np.ndarray) -> np.ndarray:
    """``v [T][N] / SA[t]`` where ``SA > 1e-8``, else ``v``."""
    ok = sa > 1e-8
    return np.where(ok[:, None], v / np.where(ok, sa, 1.0)[:, None], v)


def linear_benchmarks(batches: Dict[str, Dict], device: str = "cpu", center: str = "mean", grid=(16, 4),
                      precision: str = "bf16", thetas=None) -> Dict:
    """LS and EN benchmark SDFs of ``batches`` (``train`` / ``valid`` / ``test`` dicts of
    ``individual_features``, ``returns``, ``mask``).

    Returns ``{"LS": row, "EN": row, "candidates": {...}, "device", "center"}``. A row holds
    ``theta`` [F], ``sharpe`` / ``sharpe_unnormalised`` / ``ev`` / ``xs_r2`` (dicts by split),
    ``factor`` and ``weights`` (by split: [T] and the dense L1-normalised [T][N] float64) and, for
    EN, ``index``, ``l1``, ``l2``, ``nonzero``. ``candidates`` holds the EN grid: ``thetas`` [K][F],
    ``l1``, ``l2``, ``sweeps`` [K], and by split ``sharpe`` [K], ``ev`` [K] and ``factor`` [T][K].

    ``thetas [K][F]``: skip the estimation and select among these candidates (the two devices
    can then be compared on identical candidates); there is no LS row then."""
    for s in SPLITS:
        if s not in batches:
            raise ValueError(f"batches must hold {SPLITS}")
    bl = [batches[s] for s in SPLITS]
    F = int(bl[0]["individual_features"].shape[2])
    panel = _panel(bl, device, precision, "benchmarks")
    man = [panel.managed(s) for s in range(3)]
    cand = {}
    ls = None
    if thetas is None:
        Ft, _ = managed_factors(man[0])
        if Ft.shape[0] < 1:
            raise ValueError("the train split has no valid rows")
        A, b = en_moments(Ft)
        ls = fit_ls(Ft)
        l1s, l2s = en_grid(A, b, grid)
        ths, sweeps, pl1, pl2 = [], [], [], []
        for l2 in l2s:
            th, used = en_path(A, b, l1s, l2)
            ths.append(th); sweeps += used
            pl1 += list(l1s); pl2 += [float(l2)] * len(l1s)
        en = np.concatenate(ths, axis=0)
        cand.update(l1=np.array(pl1), l2=np.array(pl2), sweeps=np.array(sweeps, dtype=np.int64))
    else:
        en = _thetas(thetas, F).astype(np.float64)
    th32 = _thetas(en, F)
    cand["thetas"] = en
    for s, name in enumerate(SPLITS):
        sums = _chunked_sums(panel, s, th32, center_from_managed(man[s], th32, center))
        cand[name] = {"sharpe": sharpes_from_sums(sums), "ev": ev_from_sums(sums), "factor": factors_from_sums(sums)}
    best = select(cand["valid"]["sharpe"])
    rows = {"EN": en[best]} if ls is None else {"LS": ls, "EN": en[best]}
    sel = _thetas(np.stack(list(rows.values())), F)
    out = {k: {"theta": v, "sharpe": {}, "sharpe_unnormalised": {}, "ev": {}, "xs_r2": {}, "factor": {}, "weights": {}}
           for k, v in rows.items()}
    out["EN"].update(index=best, nonzero=int(np.count_nonzero(en[best])))
    if ls is not None:
        out["EN"].update(l1=float(cand["l1"][best]), l2=float(cand["l2"][best]), sweeps=int(cand["sweeps"][best]))
    gpu_ms = 0.0
    for s, name in enumerate(SPLITS):
        sums = _chunked_sums(panel, s, sel, center_from_managed(man[s], sel, center), True)
        gpu_ms += sums.get("gpu_ms", 0.0) + man[s].get("gpu_ms", 0.0)
        f, ev, sh = factors_from_sums(sums), ev_from_sums(sums), sharpes_from_sums(sums)
        Ft, keep = managed_factors(man[s])
        r, m = _np(bl[s]["returns"], np.float64), _np(bl[s]["mask"]).astype(bool)
        for k, key in enumerate(rows):
            w = _normalised(sums["v"][k], sums["sa"][:, k])
            o = out[key]
            o["sharpe"][name], o["ev"][name], o["factor"][name], o["weights"][name] = float(sh[k]), float(ev[k]), f[:, k], w
            o["sharpe_unnormalised"][name] = sharpe_ddof0(Ft @ rows[key]) if keep.size else 0.0
            o["xs_r2"][name] = cross_sectional_r2(w, r, m)
    out.update(candidates=cand, device="cuda" if isinstance(panel, _GpuPanel) else "cpu", center=center)
    if isinstance(panel, _GpuPanel):
        out["gpu_ms"] = gpu_ms
    return out


def format_benchmarks(res: Dict, gan: Optional[Dict] = None, ffn: Optional[Dict] = None,
                      ipca: Optional[Dict] = None) -> List[str]:
    """The printed table: rows LS, EN, (``ipca``: a row of ``ipca.ipca_benchmark``) IPCA,
    (``ffn``: a row of ``prediction.ffn_benchmark``) FFN and (``gan``: ``train_sharpe``,
    ``valid_sharpe``, ``test_sharpe``, ``ev``, ``xs_r2``) the GAN ensemble; columns Sharpe on train,
    valid and test, then EV and XS-R2 on test."""
    lines = [f"  {'':14s} {'SR train':>9s} {'SR valid':>9s} {'SR test':>9s} {'EV test':>9s} {'XS-R2 test':>11s}"]
    for key in ("LS", "EN"):
        if key in res:
            o = res[key]
            lines.append(f"  {key:14s} {o['sharpe']['train']:9.4f} {o['sharpe']['valid']:9.4f} {o['sharpe']['test']:9.4f} "
                         f"{o['ev']['test']:9.4f} {o['xs_r2']['test']:11.4f}")
    if ipca is not None:
        from .ipca import format_ipca_row
        lines.append(format_ipca_row(ipca))
    if ffn is not None:
        from .prediction import format_ffn_row
        lines.append(format_ffn_row(ffn))
    if gan is not None:
        lines.append(f"  {'GAN ensemble':14s} {gan['train_sharpe']:9.4f} {gan['valid_sharpe']:9.4f} {gan['test_sharpe']:9.4f} "
                     f"{gan['ev']:9.4f} {gan['xs_r2']:11.4f}")
    en = res["EN"]
    if "l1" in en:
        lines.append(f"  EN: candidate {en['index']} of {len(res['candidates']['thetas'])} (l1 {en['l1']:.3e}, l2 {en['l2']:.3e}), "
                     f"{en['nonzero']} non-zero coefficients, {en['sweeps']} sweeps; centre: {res['center']}")
    return lines


def _jsonable(v):
    if isinstance(v, np.ndarray):
        return _jsonable(v.tolist())
    if isinstance(v, dict):
        return {str(k): _jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    if isinstance(v, (float, np.floating)):
        return float(v) if np.isfinite(v) else None
    if isinstance(v, np.integer):
        return int(v)
    return v


def to_json(res: Dict, gan: Optional[Dict] = None, ffn: Optional[Dict] = None, ipca: Optional[Dict] = None) -> Dict:
    """Plain lists (non-finite values as null): every row without its dense weights, the
    candidates' penalties and Sharpe ratios, and ``gan`` / ``ffn`` (key ``FFN``) / ``ipca`` (key
    ``IPCA``) when given."""
    out = {"device": res["device"], "center": res["center"]}
    for key in ("LS", "EN"):
        if key in res:
            out[key] = _jsonable({k: v for k, v in res[key].items() if k != "weights"})
    c = res["candidates"]
    out["candidates"] = _jsonable({k: (v if k not in SPLITS else {"sharpe": v["sharpe"], "ev": v["ev"]})
                                   for k, v in c.items()})
    if ipca is not None:
        out["IPCA"] = _jsonable({k: v for k, v in ipca.items() if k != "weights"})
    if ffn is not None:
        out["FFN"] = _jsonable({k: v for k, v in ffn.items() if k != "weights"})
    if gan is not None:
        out["GAN"] = _jsonable(gan)
    return out
