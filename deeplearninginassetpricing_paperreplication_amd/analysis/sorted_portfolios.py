"""Characteristic-sorted portfolios priced by the SDF (the paper's anomaly tables and the
"predicted vs realised mean return" / "loading-sorted decile" figures).

Definition. For a period ``t`` with ``n = N_t`` valid stocks, ``Q`` buckets (``2 <= Q <= 16``) and a
key column, sort the keys ascending into ``s[0..n-1]`` (``-0.0`` equals ``+0.0``; keys of valid
rows are finite). The breakpoints are ``b_d = s[ceil(d n / Q) - 1]`` for ``d = 1..Q-1`` and

    bucket(i) = #{ d : key_i > b_d }.

Without ties this is ``floor(rank Q / n)``. Tied keys always land in the same bucket, the lowest
one any of them would get, so membership depends neither on the stock order nor on a sort's
stability (bf16 characteristics tie often). ``n < Q`` leaves some buckets empty, ``n = 0`` all.

For every (period, key, bucket) the raw result holds the row count and the float64 sums of the
value columns: the return, then the ensemble's averaged, re-normalised weight
(``portfolio.average_weights``). ``device="cpu"`` evaluates the definition with numpy (the oracle);
``device="cuda"`` runs ``Engine.sorted_portfolios`` (``csrc/k_qsort.hip``) on the panel the engine
holds in HBM. The kernel reads the panel only, so it covers every engine shape and
mixed-architecture ensembles. It sorts the characteristics as the engine stores them: bf16-rounded
by default, which moves a small share of rows next to a breakpoint into the neighbouring bucket
(README); ``precision="fp32"`` sorts the exact keys.

Pricing (``price_portfolios``) uses the project's loading convention (``portfolio`` module):
``beta_t = sum_i R w / sum_i w w`` over the valid stocks, a stock's residual is
``R_i - beta_t w_i``, and the equally weighted portfolio's residual is their mean,
``eps[t,p,q] = returns[t,p,q] - beta_t loading[t,p,q]``.

Double sorts (``double_sort_numpy`` is the definition, ``Engine.double_sorted_portfolios`` /
``csrc/k_qsort2.hip`` the GPU path). For a period with ``n`` valid stocks, a pair of key columns
``(A, B)`` and ``Qa x Qb`` buckets (``2 <= Qa, Qb <= 16``, ``Qa Qb <= 36``):

* First key: the single sort's rule. With ``s^A`` the ``n`` A-keys ascending,
  ``bA_d = s^A[ceil(d n / Qa) - 1]`` for ``d = 1..Qa-1`` and ``qa(i) = #{ d : A_i > bA_d }``.
* Independent mode: the same rule on ``B`` over all ``n`` rows with ``Qb``; one set of
  breakpoints ``bB_d`` per period, ``qb(i) = #{ d : B_i > bB_d }``.
* Conditional mode (default, the paper's dependent sort): for each first-key bucket ``a``, with
  ``S_a = { i : qa(i) = a }`` of ``n_a`` rows and ``s^{B|a}`` their B-keys ascending,
  ``bB_{a,d} = s^{B|a}[ceil(d n_a / Qb) - 1]`` and ``qb(i) = #{ d : B_i > bB_{qa(i),d} }``.
  ``n_a = 0`` leaves the cells of row ``a`` empty and its breakpoints NaN, ``n_a < Qb`` leaves
  some cells empty.
* Ties share the lowest bucket any of them would get, in both dimensions, so membership never
  depends on the stock order.
* Result per (period, pair, cell ``(qa, qb)``): the row count and the float64 sums of the value
  columns; per (period, pair): ``breaks_a`` [Qa-1] and ``breaks_b`` [Qa][Qb-1] (independent mode:
  ``Qa`` identical rows). An empty period gives zero counts and sums and NaN breakpoints.
  ``A == B`` is legal and gets no special case.

Out of scope: value-weighted buckets (the panel carries no market cap; ``sort_buckets_numpy`` and
the engine methods accept further value columns), plots (the beta network:
``analysis.prediction``). Sorts on three or more keys: ``analysis.tree_sorts``.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .portfolio import average_weights

MAX_Q = 16


def _check_q(Q: int) -> int:
    Q = int(Q)
    if Q < 2 or Q > MAX_Q:
        raise ValueError(f"quantiles must be in [2, {MAX_Q}]")
    return Q


def sort_buckets_numpy(keys: np.ndarray, mask: np.ndarray, values: np.ndarray, quantiles: int = 10) -> Dict:
    """The definition in numpy. ``keys`` [T][N][P] (float32 or float64), ``mask`` [T][N],
    ``values`` [T][N][V]. Returns ``count`` int32 [T][P][Q], ``sum`` float64 [T][P][Q][V] and
    ``breaks`` [T][P][Q-1] in the keys' dtype (NaN where the period is empty)."""
    Q = _check_q(quantiles)
    keys = np.asarray(keys)
    mask = np.asarray(mask).astype(bool)
    values = np.asarray(values)
    T, N, P = keys.shape
    V = values.shape[2]
    count = np.zeros((T, P, Q), np.int32)
    sums = np.zeros((T, P, Q, V), np.float64)
    breaks = np.full((T, P, Q - 1), np.nan, keys.dtype)
    d = np.arange(1, Q, dtype=np.int64)
    for t in range(T):
        idx = np.nonzero(mask[t])[0]
        n = int(idx.size)
        if n == 0:
            continue
        k = keys[t, idx, :] + keys.dtype.type(0)          # (-0.0 + 0.0 = +0.0)
        s = np.sort(k, axis=0)
        b = s[(d * n + Q - 1) // Q - 1, :]                # [Q-1][P]
        bucket = (k[:, None, :] > b[None, :, :]).sum(axis=1)
        v = values[t, idx, :].astype(np.float64)
        for q in range(Q):
            sel = bucket == q                             # [n][P]
            count[t, :, q] = sel.sum(axis=0)
            sums[t, :, q, :] = sel.T.astype(np.float64) @ v
        breaks[t] = b.T
    return {"count": count, "sum": sums, "breaks": breaks}


def _key_names(F: int, by_weight: bool, names: Optional[Sequence]) -> List[str]:
    ch = [str(n) for n in names] if names is not None and len(names) == F else [f"x{j}" for j in range(F)]
    return ch + (["weight"] if by_weight else [])


def _cpu_weights(models, batch) -> np.ndarray:
    from .ensemble import get_weights_from_model
    mask = batch["mask"].cpu().numpy()
    return average_weights([get_weights_from_model(m.cpu(), batch, "cpu") for m in models], mask)


def _gpu_weights(models, batch) -> torch.Tensor:
    """The averaged, re-normalised ensemble weight [T][N] (float32) on the device."""
    from .ensemble import weights_batched_gpu
    W = weights_batched_gpu(models, {"x": batch}, splits=("x",))["x"]
    m = batch["mask"].to(W.device).float()
    w = W.mean(dim=0)
    s = (w.abs().double() * m.double()).sum(dim=1, keepdim=True)
    return torch.where(s > 1e-8, (w.double() / s.clamp(min=1e-300)).float(), w).contiguous()


def _gpu_raw(spec, batch, w: torch.Tensor, Q: int, by_weight: bool, precision: str) -> Dict:
    from ..engine.runner import GANEngine
    eng = GANEngine(spec, 1, max_epochs=4, precision=precision)
    eng.set_data(batch)
    torch.cuda.synchronize(w.device)
    try:
        r = eng.eng.sorted_portfolios(0, Q, [], w.data_ptr() if by_weight else 0, 1 if by_weight else 0,
                                      w.data_ptr(), 1)
    finally:
        eng.eng.sync()
    return {"count": np.asarray(r["count"]), "sum": np.asarray(r["sum"]), "breaks": np.asarray(r["breaks"]),
            "gpu_ms": float(r["gpu_ms"])}


def sorted_portfolios(models: Sequence, batch: Dict, device: str = "cpu", quantiles: int = 10,
                      by_weight: bool = True, names: Optional[Sequence] = None,
                      weights: Optional[np.ndarray] = None, precision: str = "bf16") -> Dict:
    """Equally weighted quantile portfolios of ``batch`` on each of the F characteristics and,
    with ``by_weight``, on the ensemble weight.

    Returns ``returns`` [T][P][Q] (bucket mean return, NaN where the bucket is empty), ``loading``
    [T][P][Q] (bucket mean ensemble weight), ``count`` int32 [T][P][Q], ``breaks`` [T][P][Q-1] and
    ``names`` [P] (``names`` when given for the characteristics, else x0.., then ``weight``).

    ``weights`` [T][N]: use this ensemble weight instead of evaluating ``models`` (the two devices
    evaluate the models in different precisions; a caller comparing them passes one weight to
    both). ``precision`` is the engine's panel precision on the GPU path."""
    Q = _check_q(quantiles)
    models = list(models)
    mask = batch["mask"].bool()
    T, N, F = batch["individual_features"].shape
    gpu = str(device).startswith("cuda")
    if gpu:
        from ..ops import native
        if native.load(required=False) is None:
            print("[sorted_portfolios] native extension not available: using the CPU path")
            gpu = False
    if not models and (weights is None or gpu):      # (the engine is built from a model's spec)
        raise ValueError("no models")
    if gpu:
        dev = torch.device("cuda", torch.cuda.current_device())
        if weights is None:
            w = _gpu_weights(models, batch)
        else:
            w = torch.as_tensor(np.asarray(weights, dtype=np.float32)).to(dev).contiguous()
        raw = _gpu_raw(models[0].spec, batch, w, Q, by_weight, precision)
    else:
        cpu = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
        w = _cpu_weights(models, cpu) if weights is None else np.asarray(weights)
        w = w.astype(np.float32)
        keys = cpu["individual_features"].numpy().astype(np.float32)
        if by_weight:
            keys = np.concatenate([keys, w[:, :, None]], axis=2)
        vals = np.stack([cpu["returns"].numpy().astype(np.float32), w], axis=2)
        raw = sort_buckets_numpy(keys, mask.cpu().numpy(), vals, Q)
    cnt = raw["count"]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(cnt[..., None] > 0, raw["sum"] / cnt[..., None], np.nan)
    out = {"returns": mean[..., 0], "loading": mean[..., 1], "count": cnt, "breaks": raw["breaks"],
           "names": _key_names(F, by_weight, names), "quantiles": Q}
    if "gpu_ms" in raw:
        out["gpu_ms"] = raw["gpu_ms"]
    return out


def price_portfolios(res: Dict, weights: np.ndarray, returns: np.ndarray, mask: np.ndarray) -> Dict:
    """Price the ``P * Q`` test assets of ``res`` with the SDF weight ``weights`` [T][N].

    Per asset, over its non-empty periods (all [P][Q]): ``mean_ret``, ``alpha`` (mean residual),
    ``t_alpha`` (alpha over its standard error, sample standard deviation; NaN with fewer than two
    periods) and ``ev = 1 - sum eps^2 / sum ret^2``. Per key ([P]): ``hml`` and ``hml_sharpe``, the
    mean and the Sharpe ratio (population standard deviation, as the project's Sharpe ratios) of
    the highest-minus-lowest bucket return over the periods where both are non-empty. Overall,
    over the assets with at least one period: ``ev = 1 - sum_a mean_t eps^2 / sum_a mean_t ret^2``,
    ``xs_r2 = 1 - mean(alpha^2) / mean(mean_ret^2)`` and ``mean_abs_alpha``."""
    m = np.asarray(mask).astype(np.float64)
    w = np.asarray(weights).astype(np.float64) * m
    r = np.asarray(returns).astype(np.float64) * m
    ww = (w * w).sum(axis=1)
    rw = (r * w).sum(axis=1)
    beta = np.divide(rw, ww, out=np.zeros_like(rw), where=ww > 1e-12)       # as _projection_residuals
    ok = np.asarray(res["count"]) > 0
    ret = np.where(ok, res["returns"], 0.0)
    eps = np.where(ok, ret - beta[:, None, None] * np.where(ok, res["loading"], 0.0), 0.0)
    nt = ok.sum(axis=0).astype(np.float64)
    has = nt > 0
    den = np.maximum(nt, 1.0)
    nan = np.full(nt.shape, np.nan)
    mean_ret = np.where(has, ret.sum(axis=0) / den, nan)
    alpha = np.where(has, eps.sum(axis=0) / den, nan)
    dev = np.where(ok, eps - np.where(has, alpha, 0.0)[None], 0.0)
    var = np.divide((dev * dev).sum(axis=0), nt - 1.0, out=nan.copy(), where=nt > 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        t_alpha = np.where(var > 0, alpha / np.sqrt(var / den), np.nan)
    r2 = (ret * ret).sum(axis=0)
    e2 = (eps * eps).sum(axis=0)
    ev = np.divide(e2, r2, out=nan.copy(), where=r2 > 0)
    ev = 1.0 - ev
    both = ok[:, :, 0] & ok[:, :, -1]
    spread = np.where(both, ret[:, :, -1] - ret[:, :, 0], 0.0)
    nb = both.sum(axis=0).astype(np.float64)
    hml = np.divide(spread.sum(axis=0), nb, out=np.full(nb.shape, np.nan), where=nb > 0)
    sd = np.sqrt(np.divide((np.where(both, spread - np.where(nb > 0, hml, 0.0)[None], 0.0) ** 2).sum(axis=0), nb,
                           out=np.full(nb.shape, np.nan), where=nb > 0))
    with np.errstate(invalid="ignore", divide="ignore"):
        hml_sharpe = np.where(sd > 0, hml / sd, np.nan)
    me2, mr2 = (e2 / den)[has], (r2 / den)[has]
    overall_ev = float(1.0 - me2.sum() / mr2.sum()) if has.any() and mr2.sum() > 0 else float("nan")
    a, mr = alpha[has], mean_ret[has]
    mm = float((mr * mr).mean()) if has.any() else 0.0
    return {"mean_ret": mean_ret, "alpha": alpha, "t_alpha": t_alpha, "ev_asset": ev, "hml": hml,
            "hml_sharpe": hml_sharpe, "ev": overall_ev,
            "xs_r2": float(1.0 - (a * a).mean() / mm) if mm > 0 else float("nan"),
            "mean_abs_alpha": float(np.abs(a).mean()) if has.any() else float("nan"),
            "assets": int(has.sum()), "names": list(res["names"])}


def format_sorted(priced: Dict, top: int = 10) -> List[str]:
    """The printed report: the overall line, the weight-sorted bucket mean returns with H-L, and
    the ``top`` characteristics with the largest |H-L|."""
    names = priced["names"]
    P, Q = priced["mean_ret"].shape
    lines = [f"  {priced['assets']} test assets ({P} keys x {Q} buckets):  EV {priced['ev']:7.4f}  "
             f"XS-R2 {priced['xs_r2']:7.4f}  mean |alpha| {priced['mean_abs_alpha']:.3e}"]
    nchar = P
    if names and names[-1] == "weight":
        nchar = P - 1
        lines.append("  Sorted on the ensemble weight, bucket mean returns (low .. high), H-L, Sharpe:")
        lines.append("    " + " ".join(f"{v: .4f}" for v in priced["mean_ret"][-1])
                     + f"   H-L {priced['hml'][-1]: .4f}  SR {priced['hml_sharpe'][-1]: .3f}")
    h = np.nan_to_num(np.abs(priced["hml"][:nchar]), nan=-1.0)
    order = np.argsort(-h, kind="stable")[:top]
    lines.append(f"  Top {len(order)} characteristics by |H-L| (H-L, Sharpe, low and high bucket mean return):")
    lines += [f"    {k + 1:2d}. {names[j]:<16s} {priced['hml'][j]: .4f}  {priced['hml_sharpe'][j]: .3f}  "
              f"{priced['mean_ret'][j][0]: .4f}  {priced['mean_ret'][j][-1]: .4f}" for k, j in enumerate(order)]
    return lines


def _jsonable(v):
    if isinstance(v, np.ndarray):
        return _jsonable(v.tolist())
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    if isinstance(v, (float, np.floating)):
        return float(v) if np.isfinite(v) else None
    if isinstance(v, np.integer):
        return int(v)
    return v


def to_json(res: Dict, priced: Optional[Dict] = None) -> Dict:
    """Plain lists (non-finite values as null): the time means of ``res`` per asset, its counts
    summed over the periods, and every key of ``priced``."""
    out = {"names": list(res["names"]), "quantiles": int(res["quantiles"]),
           "periods": int(res["count"].shape[0]), "count": _jsonable(res["count"].sum(axis=0))}
    if priced is not None:
        out.update({k: _jsonable(v) for k, v in priced.items()})
    return out


# ---------------------------------------------------------------------------------------------
# Double sorts (definition in the module docstring)

MAX_CELLS = 36
MAX_DOUBLE_VALUES = 2


def _check_q2(quantiles) -> tuple:
    try:
        qa, qb = quantiles
    except (TypeError, ValueError):
        raise ValueError("quantiles must be a pair (Qa, Qb)") from None
    Qa, Qb = _check_q(qa), _check_q(qb)
    if Qa * Qb > MAX_CELLS:
        raise ValueError(f"Qa * Qb must be at most {MAX_CELLS}")
    return Qa, Qb


def parse_double_quantiles(spec) -> tuple:
    """CLI form of ``quantiles``: ``"5x5"`` (or a pair, returned checked)."""
    if isinstance(spec, str):
        ab = spec.lower().split("x")
        if len(ab) != 2:
            raise ValueError(f"double_quantiles: expected QAxQB, got {spec!r}")
        try:
            spec = (int(ab[0]), int(ab[1]))
        except ValueError:
            raise ValueError(f"double_quantiles: expected QAxQB, got {spec!r}") from None
    return _check_q2(spec)


def _breaks(sorted_keys: np.ndarray, Q: int) -> np.ndarray:
    n = sorted_keys.shape[0]
    d = np.arange(1, Q, dtype=np.int64)
    return sorted_keys[(d * n + Q - 1) // Q - 1]


def double_sort_numpy(keys: np.ndarray, pairs: Sequence, mask: np.ndarray, values: np.ndarray,
                      quantiles=(5, 5), conditional: bool = True) -> Dict:
    """The definition in numpy. ``keys`` [T][N][P'] (float32 or float64), ``pairs`` a list of
    (A, B) columns of ``keys``, ``mask`` [T][N], ``values`` [T][N][V]. Returns ``count`` int32
    [T][P][Qa][Qb], ``sum`` float64 [T][P][Qa][Qb][V], ``breaks_a`` [T][P][Qa-1] and ``breaks_b``
    [T][P][Qa][Qb-1] in the keys' dtype (NaN where the period, or the first-key bucket, is empty)
    and ``rows``."""
    Qa, Qb = _check_q2(quantiles)
    keys = np.asarray(keys)
    mask = np.asarray(mask).astype(bool)
    values = np.asarray(values)
    T, N, PK = keys.shape
    V = values.shape[2]
    pairs = [(int(a), int(b)) for a, b in pairs]
    for a, b in pairs:
        if not (0 <= a < PK and 0 <= b < PK):
            raise ValueError(f"pair ({a}, {b}) outside the {PK} key columns")
    P = len(pairs)
    count = np.zeros((T, P, Qa, Qb), np.int32)
    sums = np.zeros((T, P, Qa, Qb, V), np.float64)
    breaks_a = np.full((T, P, Qa - 1), np.nan, keys.dtype)
    breaks_b = np.full((T, P, Qa, Qb - 1), np.nan, keys.dtype)
    zero = keys.dtype.type(0)
    for t in range(T):
        idx = np.nonzero(mask[t])[0]
        n = int(idx.size)
        if n == 0:
            continue
        v = values[t, idx, :].astype(np.float64)
        for p, (ca, cb) in enumerate(pairs):
            kA = keys[t, idx, ca] + zero                      # (-0.0 + 0.0 = +0.0)
            kB = keys[t, idx, cb] + zero
            bA = _breaks(np.sort(kA), Qa)
            qa = (kA[:, None] > bA[None, :]).sum(axis=1)
            breaks_a[t, p] = bA
            qb = np.zeros(n, np.int64)
            if conditional:
                for a in range(Qa):
                    sel = qa == a
                    if not sel.any():
                        continue
                    bB = _breaks(np.sort(kB[sel]), Qb)
                    breaks_b[t, p, a] = bB
                    qb[sel] = (kB[sel][:, None] > bB[None, :]).sum(axis=1)
            else:
                bB = _breaks(np.sort(kB), Qb)
                breaks_b[t, p, :] = bB[None, :]
                qb = (kB[:, None] > bB[None, :]).sum(axis=1)
            cell = qa * Qb + qb
            onehot = (cell[None, :] == np.arange(Qa * Qb)[:, None]).astype(np.float64)   # [cells][n]
            count[t, p] = onehot.sum(axis=1).astype(np.int32).reshape(Qa, Qb)
            sums[t, p] = (onehot @ v).reshape(Qa, Qb, V)
    return {"count": count, "sum": sums, "breaks_a": breaks_a, "breaks_b": breaks_b, "rows": int(mask.sum())}


def _resolve_pairs(pairs: Sequence, F: int, names: Optional[Sequence]) -> List[tuple]:
    """Pair members as key indices: a column in [0, F), or ``F`` / ``"weight"`` for the ensemble
    weight (a characteristic's name when ``names`` is given)."""
    idx = {str(nm): i for i, nm in enumerate(names)} if names is not None and len(names) == F else {}

    def one(m):
        if isinstance(m, str):
            if m == "weight":
                return F
            if m in idx:
                return idx[m]
            try:
                m = int(m)
            except ValueError:
                raise ValueError(f"double sorts: unknown key {m!r}") from None
        m = int(m)
        if m < 0 or m > F:
            raise ValueError(f"double sorts: key {m} outside [0, {F}] ({F} is the weight)")
        return m
    out = []
    for pr in pairs:
        if len(pr) != 2:
            raise ValueError(f"double sorts: expected a pair, got {pr!r}")
        out.append((one(pr[0]), one(pr[1])))
    return out


def _gpu_raw2(spec, batch, w: torch.Tensor, pairs, Qa: int, Qb: int, conditional: bool, precision: str) -> Dict:
    from ..engine.runner import GANEngine
    eng = GANEngine(spec, 1, max_epochs=4, precision=precision)
    eng.set_data(batch)
    torch.cuda.synchronize(w.device)
    try:
        r = eng.eng.double_sorted_portfolios(0, [tuple(p) for p in pairs], Qa, Qb, bool(conditional),
                                             w.data_ptr(), 1, w.data_ptr(), 1)
    finally:
        eng.eng.sync()
    out = {k: np.asarray(r[k]) for k in ("count", "sum", "breaks_a", "breaks_b")}
    out["gpu_ms"] = float(r["gpu_ms"])
    return out


def double_sorted_portfolios(models: Sequence, batch: Dict, pairs: Sequence, device: str = "cpu",
                             quantiles=(5, 5), conditional: bool = True, names: Optional[Sequence] = None,
                             weights: Optional[np.ndarray] = None, precision: str = "bf16") -> Dict:
    """Equally weighted ``Qa x Qb`` double-sorted portfolios of ``batch`` for every pair of
    ``pairs``: members are column indices (or names, with ``names``), or ``F`` / ``"weight"`` for
    the ensemble weight (on the GPU the weight is the engine method's one extra key).

    Returns ``returns`` and ``loading`` [T][P][Qa][Qb] (cell mean return / ensemble weight, NaN
    where the cell is empty), ``count`` int32 [T][P][Qa][Qb], ``breaks_a`` [T][P][Qa-1],
    ``breaks_b`` [T][P][Qa][Qb-1], ``pairs`` (resolved indices), ``names`` (``"A x B"``),
    ``quantiles`` (Qa, Qb), ``mode`` and, on the GPU, ``gpu_ms``. ``weights`` and ``precision`` as
    for ``sorted_portfolios``."""
    Qa, Qb = _check_q2(quantiles)
    models = list(models)
    mask = batch["mask"].bool()
    T, N, F = batch["individual_features"].shape
    prs = _resolve_pairs(pairs, F, names)
    gpu = str(device).startswith("cuda")
    if gpu:
        from ..ops import native
        if native.load(required=False) is None:
            print("[sorted_portfolios] native extension not available: using the CPU path")
            gpu = False
    if not models and (weights is None or gpu):      # (the engine is built from a model's spec)
        raise ValueError("no models")
    if gpu:
        dev = torch.device("cuda", torch.cuda.current_device())
        if weights is None:
            w = _gpu_weights(models, batch)
        else:
            w = torch.as_tensor(np.asarray(weights, dtype=np.float32)).to(dev).contiguous()
        raw = _gpu_raw2(models[0].spec, batch, w, prs, Qa, Qb, conditional, precision)
    else:
        cpu = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
        w = _cpu_weights(models, cpu) if weights is None else np.asarray(weights)
        w = w.astype(np.float32)
        keys = np.concatenate([cpu["individual_features"].numpy().astype(np.float32), w[:, :, None]], axis=2)
        vals = np.stack([cpu["returns"].numpy().astype(np.float32), w], axis=2)
        raw = double_sort_numpy(keys, prs, mask.cpu().numpy(), vals, (Qa, Qb), conditional)
    cnt = raw["count"]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(cnt[..., None] > 0, raw["sum"] / cnt[..., None], np.nan)
    kn = _key_names(F, True, names)
    out = {"returns": mean[..., 0], "loading": mean[..., 1], "count": cnt, "breaks_a": raw["breaks_a"],
           "breaks_b": raw["breaks_b"], "pairs": prs, "names": [f"{kn[a]} x {kn[b]}" for a, b in prs],
           "quantiles": (Qa, Qb), "mode": "conditional" if conditional else "independent"}
    if "gpu_ms" in raw:
        out["gpu_ms"] = raw["gpu_ms"]
    return out


def price_double_sorted(res: Dict, weights: np.ndarray, returns: np.ndarray, mask: np.ndarray) -> Dict:
    """Price the ``P * Qa * Qb`` test assets of ``res`` (``double_sorted_portfolios``) with the SDF
    weight ``weights`` [T][N]: the cells are flattened to [T][P][Qa Qb] and priced by
    ``price_portfolios``.

    Per asset ([P][Qa][Qb]): ``mean_ret``, ``alpha``, ``t_alpha``, ``ev_asset``. Per pair ([P], over
    the pair's non-empty cells, the formulas of ``price_portfolios``' overall numbers; the paper's
    per-table figures): ``pair_ev``, ``pair_xs_r2``, ``pair_mean_abs_alpha``, and the corner spread
    cell(Qa-1, Qb-1) - cell(0, 0) over the periods where both exist, ``hml`` with its Sharpe ratio
    ``hml_sharpe``. Over all pairs: ``ev``, ``xs_r2``, ``mean_abs_alpha``, ``assets``."""
    cnt = np.asarray(res["count"])
    T, P, Qa, Qb = cnt.shape

    def flat(sel):
        return {"names": list(res["names"])[sel],
                **{k: np.asarray(res[k])[:, sel].reshape(T, -1, Qa * Qb) for k in ("count", "returns", "loading")}}
    allp = price_portfolios(flat(slice(None)), weights, returns, mask)
    out = {k: allp[k].reshape(P, Qa, Qb) for k in ("mean_ret", "alpha", "t_alpha", "ev_asset")}
    per = [price_portfolios(flat(slice(p, p + 1)), weights, returns, mask) for p in range(P)]
    out.update({"pair_ev": np.array([q["ev"] for q in per], np.float64),
                "pair_xs_r2": np.array([q["xs_r2"] for q in per], np.float64),
                "pair_mean_abs_alpha": np.array([q["mean_abs_alpha"] for q in per], np.float64),
                "hml": allp["hml"], "hml_sharpe": allp["hml_sharpe"], "ev": allp["ev"], "xs_r2": allp["xs_r2"],
                "mean_abs_alpha": allp["mean_abs_alpha"], "assets": allp["assets"], "names": list(res["names"]),
                "quantiles": tuple(res["quantiles"]), "mode": res["mode"]})
    return out


def format_double_sorted(priced: Dict) -> List[str]:
    """The printed report: the overall line, then per pair its EV / XS-R2 / mean |alpha|, the corner
    spread with its Sharpe ratio, and the Qa x Qb table of cell mean returns (rows: first key)."""
    P, Qa, Qb = priced["mean_ret"].shape
    lines = [f"  {priced['assets']} test assets ({P} pairs x {Qa} x {Qb} cells, {priced['mode']}):  "
             f"EV {priced['ev']:7.4f}  XS-R2 {priced['xs_r2']:7.4f}  mean |alpha| {priced['mean_abs_alpha']:.3e}"]
    for p, name in enumerate(priced["names"]):
        lines.append(f"  {name}:  EV {priced['pair_ev'][p]:7.4f}  XS-R2 {priced['pair_xs_r2'][p]:7.4f}  "
                     f"mean |alpha| {priced['pair_mean_abs_alpha'][p]:.3e}  corner H-L {priced['hml'][p]: .4f}  "
                     f"SR {priced['hml_sharpe'][p]: .3f}")
        lines += ["    " + " ".join(f"{v: .4f}" for v in row) for row in priced["mean_ret"][p]]
    return lines


def double_to_json(res: Dict, priced: Optional[Dict] = None) -> Dict:
    """Plain lists (non-finite values as null): the counts of ``res`` summed over the periods and
    every key of ``priced``."""
    out = {"names": list(res["names"]), "pairs": [list(p) for p in res["pairs"]],
           "quantiles": [int(q) for q in res["quantiles"]], "mode": res["mode"],
           "periods": int(res["count"].shape[0]), "count": _jsonable(res["count"].sum(axis=0))}
    if priced is not None:
        out.update({k: _jsonable(v) for k, v in priced.items()})
    return out
