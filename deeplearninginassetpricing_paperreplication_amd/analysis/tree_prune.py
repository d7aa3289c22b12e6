"""Pruning the tree-sorted portfolios into an SDF: the elastic-net mean-variance step of the
asset-pricing trees of Bryzgalova, Pelger and Zhu. The nodes of ``analysis.tree_sorts`` are the assets;
a grid of penalties (mean shrinkage ``l0``, ridge ``l2``, a descending ``l1`` path) gives candidate
sparse mean-variance weights on the train split, the validation Sharpe ratio picks one.

The estimator (``en_paths_numpy`` is the oracle, ``csrc/k_encd.hip`` the GPU path). Inputs ``A``
[NA][n][n] float64, every matrix bitwise symmetric, and per path ``p`` the matrix ``a_of[p]``, ``b[p]``
[n], the penalties ``l1s[p]`` [n1] in the order they are run and ``l2[p]``. With ``M = A[a_of[p]]`` and
``diag[j] = M[j][j] + l2`` the path starts from ``th = 0``, ``g = 0``; ``g`` (``= M th`` up to rounding)
is carried along the whole path and never recomputed, which is the one deliberate difference from
``benchmarks.en_path`` (whose ``A @ th`` through BLAS has no defined order). For each ``l1`` sweeps
``1 .. max_sweeps`` run over ``j = 0 .. n-1``::

    rho = b[j] - (g[j] - M[j][j] * th[j])                      every operation rounded once, no fma
    new = copysign(max(|rho| - l1, 0), rho) / diag[j]   if diag[j] > 0 else 0.0
    d   = new - th[j]
    if d != 0:  g[i] = g[i] + (M[i][j] * d) for all i;  th[j] = new;  step = max(step, |d|)

A sweep ends the point when ``step <= 1e-10 * max(1.0, max_j |th_j|)`` (``step`` is reset per sweep).
``theta[p][k] = th``, ``sweeps[p][k]`` and ``nnz[p][k] = #{th != 0}`` are recorded. With ``max_assets``
a finished point with ``nnz > max_assets`` is kept and ends the path: the later points are not
computed and keep ``sweeps = 0``, zero rows and ``nnz = 0``.

A coordinate with ``d == 0`` changes nothing, so the loop may jump: evaluate ``d`` for all ``j >= j0``
at once, apply the lowest ``j`` with ``d != 0`` and go on from ``j + 1``. ``en_paths_numpy`` and the
kernel both do that, ``en_path_loop`` is the loop as written above; all three give the same bits.

Limits: ``n <= 4096`` on the GPU (above it ``en_paths`` runs numpy and says so); finite inputs,
``l1, l2 >= 0``.

Stock-level weights. A node is an equally weighted basket, so the pruned SDF ``F_t = R_t . theta`` is
a weight per stock-month: ``node_coefficients`` scatters ``theta`` (times ``node_returns``' depth factor)
to the nodes, ``pruned_weights`` walks every stock down the selected trees (``tree_sorts.tree_weights``,
``csrc/k_qtree_weight.hip`` on the GPU) and returns the dense ``w`` [T][N] with ``sum_i w R = F_t``, which
``portfolio.paper_metrics`` and the pricing functions take like any other model's weight.

Out of scope: value weighting, LARS, cross-validation folds, the elastic net of ``analysis.benchmarks``
through the kernel, plots, multi-rank runs.
"""
from __future__ import annotations

import time
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import tree_sorts as ts
from .portfolio import sharpe_ddof0
from .sorted_portfolios import _jsonable

EN_TOL = 1e-10
SPLITS = ("train", "valid", "test")


def _host(x, dtype) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x), dtype=dtype)


def _check_shapes(A, a_of, b, l1s, l2):
    if A.ndim != 3 or A.shape[1] != A.shape[2] or A.shape[0] < 1 or A.shape[1] < 1:
        raise ValueError("en_paths: A must be [NA][n][n] with NA, n >= 1")
    NA, n = int(A.shape[0]), int(A.shape[1])
    if b.ndim != 2 or b.shape[1] != n or b.shape[0] < 1:
        raise ValueError("en_paths: b must be [P][n] with P >= 1")
    P = int(b.shape[0])
    if l1s.ndim != 2 or l1s.shape[0] != P or l1s.shape[1] < 1:
        raise ValueError("en_paths: l1s must be [P][n1] with n1 >= 1")
    if tuple(l2.shape) != (P,) or tuple(a_of.shape) != (P,):
        raise ValueError("en_paths: l2 and a_of must be [P]")
    return NA, P, n, int(l1s.shape[1])


def _check_values(A, a_of, b, l1s, l2, NA) -> None:
    """``A`` .. ``l2`` as numpy arrays or as tensors of one device."""
    if isinstance(A, torch.Tensor):
        fin = all(bool(torch.isfinite(x).all()) for x in (A, b, l1s, l2))
        sym = bool(torch.equal(A.view(torch.int64), A.transpose(1, 2).contiguous().view(torch.int64)))
        neg = bool((l1s < 0).any()) or bool((l2 < 0).any())
        bad = bool((a_of < 0).any()) or bool((a_of >= NA).any())
    else:
        fin = all(bool(np.isfinite(x).all()) for x in (A, b, l1s, l2))
        sym = bool(np.array_equal(A.view(np.uint64), np.ascontiguousarray(A.transpose(0, 2, 1)).view(np.uint64)))
        neg = bool((l1s < 0).any()) or bool((l2 < 0).any())
        bad = bool((a_of < 0).any()) or bool((a_of >= NA).any())
    if not fin:
        raise ValueError("en_paths: non-finite input")
    if not sym:
        raise ValueError("en_paths: every matrix of A must be bitwise symmetric")
    if neg:
        raise ValueError("en_paths: l1 and l2 must be non-negative")
    if bad:
        raise ValueError(f"en_paths: a_of outside [0, {NA})")


def _check_limits(max_sweeps, max_assets):
    max_sweeps = int(max_sweeps)
    if max_sweeps < 1:
        raise ValueError("en_paths: max_sweeps must be at least 1")
    if max_assets is not None:
        max_assets = int(max_assets)
        if max_assets < 0:
            raise ValueError("en_paths: max_assets must be non-negative")
    return max_sweeps, max_assets


def _soft(rho, l1, diag):
    """``new`` of the definition for arrays (``diag <= 0`` gives 0.0)."""
    pos = diag > 0
    return np.where(pos, np.copysign(np.maximum(np.abs(rho) - l1, 0.0), rho) / np.where(pos, diag, 1.0), 0.0)


def en_path_loop(M: np.ndarray, b: np.ndarray, l1s: Sequence[float], l2: float, max_sweeps: int = 2000,
                 max_assets: Optional[int] = None):
    """One path by the loop of the definition, coordinate by coordinate in Python floats (slow: the
    cross-check of the jump form). Returns ``(theta [n1][n], sweeps [n1], nnz [n1], updates [n1])``."""
    M = np.asarray(M, dtype=np.float64)
    n = M.shape[0]
    Ml = M.tolist()
    bl = [float(x) for x in b]
    l2 = float(l2)
    dm = [Ml[j][j] for j in range(n)]
    diag = [dm[j] + l2 for j in range(n)]
    th, g = [0.0] * n, np.zeros(n)
    n1 = len(l1s)
    theta, used, nnz, ups = np.zeros((n1, n)), np.zeros(n1, np.int32), np.zeros(n1, np.int32), np.zeros(n1, np.int64)
    for k in range(n1):
        l1 = float(l1s[k])
        sweeps = 0
        while sweeps < max_sweeps:
            sweeps += 1
            step = 0.0
            for j in range(n):
                rho = bl[j] - (float(g[j]) - dm[j] * th[j])
                new = float(np.copysign(max(abs(rho) - l1, 0.0), rho)) / diag[j] if diag[j] > 0 else 0.0
                d = new - th[j]
                if d != 0.0:
                    g = g + M[:, j] * d
                    th[j] = new
                    step = max(step, abs(d))
                    ups[k] += 1
            if step <= EN_TOL * max(1.0, max(abs(t) for t in th)):
                break
        theta[k] = th
        used[k] = sweeps
        nnz[k] = sum(1 for t in th if t != 0.0)
        if max_assets is not None and nnz[k] > max_assets:
            break
    return theta, used, nnz, ups


def _path_numpy(M, b, l1s, l2, max_sweeps, max_assets):
    n = b.shape[0]
    dm = np.ascontiguousarray(np.diagonal(M))
    diag = dm + l2
    th, g = np.zeros(n), np.zeros(n)
    n1 = l1s.shape[0]
    theta, used, nnz, ups = np.zeros((n1, n)), np.zeros(n1, np.int32), np.zeros(n1, np.int32), np.zeros(n1, np.int64)
    for k in range(n1):
        l1 = float(l1s[k])
        sweeps = 0
        while sweeps < max_sweeps:
            sweeps += 1
            step, j0 = 0.0, 0
            while j0 < n:                                  # the lowest j >= j0 whose value changes
                t = th[j0:]
                new = _soft(b[j0:] - (g[j0:] - dm[j0:] * t), l1, diag[j0:])
                d = new - t
                nz = np.flatnonzero(d)
                if nz.size == 0:
                    break
                i = int(nz[0])
                j = j0 + i
                g += M[j] * d[i]                           # (column j of the symmetric M is its row j)
                th[j] = new[i]
                step = max(step, abs(float(d[i])))
                ups[k] += 1
                j0 = j + 1
            if step <= EN_TOL * max(1.0, float(np.abs(th).max())):
                break
        theta[k] = th
        used[k] = sweeps
        nnz[k] = int(np.count_nonzero(th))
        if max_assets is not None and nnz[k] > max_assets:
            break
    return theta, used, nnz, ups


def en_paths_numpy(A, a_of, b, l1s, l2, max_sweeps: int = 2000, max_assets: Optional[int] = None) -> Dict:
    """The definition (module docstring) in numpy, in its jump form. Returns ``theta`` float64
    [P][n1][n], ``sweeps`` and ``nnz`` int32 [P][n1] and ``updates`` int64 [P][n1] (the coordinate
    updates of every point)."""
    A, b, l1s, l2 = _host(A, np.float64), _host(b, np.float64), _host(l1s, np.float64), _host(l2, np.float64)
    a_of = _host(a_of, np.int64)
    NA, P, n, n1 = _check_shapes(A, a_of, b, l1s, l2)
    _check_values(A, a_of, b, l1s, l2, NA)
    max_sweeps, max_assets = _check_limits(max_sweeps, max_assets)
    out = {"theta": np.zeros((P, n1, n)), "sweeps": np.zeros((P, n1), np.int32), "nnz": np.zeros((P, n1), np.int32),
           "updates": np.zeros((P, n1), np.int64)}
    for p in range(P):
        r = _path_numpy(A[int(a_of[p])], b[p], l1s[p], float(l2[p]), max_sweeps, max_assets)
        for key, v in zip(("theta", "sweeps", "nnz", "updates"), r):
            out[key][p] = v
    return out


def _en_paths_device(nat, dev, A, a_of, b, l1s, l2, max_sweeps, max_assets, sweeps_per_launch) -> Dict:
    def on(x, dtype):
        if isinstance(x, torch.Tensor):
            return x.detach().to(device=dev, dtype=dtype).contiguous()     # (a tensor that fits is used where it lies)
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype={torch.float64: np.float64, torch.int32: np.int32}[dtype])).to(dev)
    Ad, bd, l1d, l2d, ad = on(A, torch.float64), on(b, torch.float64), on(l1s, torch.float64), on(l2, torch.float64), on(a_of, torch.int32)
    NA, P, n, n1 = _check_shapes(Ad, ad, bd, l1d, l2d)
    _check_values(Ad, ad, bd, l1d, l2d, NA)
    theta = torch.empty((P, n1, n), dtype=torch.float64, device=dev)
    sweeps = torch.empty((P, n1), dtype=torch.int32, device=dev)
    nnz = torch.empty((P, n1), dtype=torch.int32, device=dev)
    state = torch.empty(nat.encd_state_bytes(P, n) // 8, dtype=torch.float64, device=dev)
    spl = int(nat.ENCD_DEFAULT_SWEEPS_PER_LAUNCH if sweeps_per_launch is None else sweeps_per_launch)
    if spl < 1:
        raise ValueError("en_paths: sweeps_per_launch must be at least 1")
    with torch.cuda.device(dev):
        r = nat.en_paths(Ad.data_ptr(), ad.data_ptr(), bd.data_ptr(), l1d.data_ptr(), l2d.data_ptr(), theta.data_ptr(),
                         sweeps.data_ptr(), nnz.data_ptr(), state.data_ptr(), NA, P, n, n1, max_sweeps,
                         -1 if max_assets is None else max_assets, spl, torch.cuda.current_stream(dev).cuda_stream)
    return {"theta": theta.cpu().numpy(), "sweeps": sweeps.cpu().numpy(), "nnz": nnz.cpu().numpy(),
            "path_updates": np.asarray(r["updates"], dtype=np.int64), "launches": int(r["launches"]),
            "launch_ms": [float(x) for x in r["launch_ms"]], "gpu_ms": float(sum(r["launch_ms"]))}


def en_paths(A, a_of, b, l1s, l2, max_sweeps: int = 2000, max_assets: Optional[int] = None, device=None,
             sweeps_per_launch: Optional[int] = None) -> Dict:
    """``en_paths_numpy`` on the CPU or ``k_encd`` on the GPU, with the same bits. ``A`` .. ``l2`` may be
    arrays or tensors; float64 (``a_of`` int32) contiguous tensors of the device are read where they lie
    and are not written. ``device``: ``None`` / ``"auto"`` (the GPU when there is one), ``"cpu"``,
    ``"cuda[:k]"``. With a GPU the native extension has to load: there is no eager fallback; only an
    ``n`` outside ``encd_supported`` goes to numpy, with a printed note.

    Returns ``theta``, ``sweeps``, ``nnz`` as numpy arrays; from the kernel also ``gpu_ms`` (the device
    time of all launches), ``launch_ms``, ``launches`` and ``path_updates`` [P]; from numpy ``updates``
    [P][n1]. A launch runs at most ``sweeps_per_launch`` sweeps of a path (default
    ``ENCD_DEFAULT_SWEEPS_PER_LAUNCH``); no output bit depends on it."""
    from ..data.transforms import _resolve_device
    max_sweeps, max_assets = _check_limits(max_sweeps, max_assets)
    if device is None and isinstance(A, torch.Tensor) and A.is_cuda:
        device = A.device
    dev = _resolve_device(device)
    if dev is not None:
        from ..ops import native
        nat = native.load(required=True)
        n = int(A.shape[-1])
        if nat.encd_supported(n):
            return _en_paths_device(nat, dev, A, a_of, b, l1s, l2, max_sweeps, max_assets, sweeps_per_launch)
        print(f"[en_paths] n = {n} is outside encd_supported (1 .. {nat.ENCD_MAX_N}): using the numpy path")
    return en_paths_numpy(A, a_of, b, l1s, l2, max_sweeps, max_assets)


# ---- the pruning pipeline (host float64) ----------------------------------------------------------
def node_returns(res: Dict, depth_weight: bool = True):
    """The assets of the pruning step: the distinct nodes (``tree_sorts.unique_nodes``, the root
    included) of a ``tree_sorted_portfolios`` result. Returns ``(R, un)``: ``R`` float64 [T][n], the node
    mean return with 0 where the node is empty, times ``1 / sqrt(nodes_per_level[level])`` with
    ``depth_weight``; ``un`` the ``unique_nodes`` dict (``nodes``, ``levels``, ``leaves``)."""
    un = ts.unique_nodes(res["trees"], res["splits"])
    if not un["nodes"]:
        raise ValueError("tree prune: no nodes")
    pi, ni = np.array([p for p, _ in un["nodes"]]), np.array([j for _, j in un["nodes"]])
    R = np.nan_to_num(np.asarray(res["returns"], dtype=np.float64)[:, pi, ni], nan=0.0)
    if depth_weight:
        npl = np.asarray(ts.tree_layout(res["splits"])["nodes_per_level"], dtype=np.float64)
        R = R * (1.0 / np.sqrt(npl[np.asarray(un["levels"])]))[None, :]
    return R, un


def mv_moments(R: np.ndarray):
    """``mu = mean_t R`` and ``S = R'R / T - mu mu'`` with the upper triangle mirrored, so that ``S`` is
    bitwise symmetric."""
    R = np.asarray(R, dtype=np.float64)
    if R.ndim != 2 or R.shape[0] < 1:
        raise ValueError("mv_moments: R must be [T][n] with T >= 1")
    mu = R.mean(axis=0)
    S = R.T @ R / R.shape[0] - np.outer(mu, mu)
    S = np.triu(S) + np.triu(S, 1).T
    return mu, S


PRUNE_L0 = (0.0, 0.25, 0.5)
PRUNE_L2_REL = (1e-3, 1e-2, 1e-1)


def parse_prune_grid(spec) -> tuple:
    """CLI form of the grid: ``"3x3x16"`` = the first 3 of ``l0``, the first 3 of ``l2_rel``, ``n1 = 16``."""
    if isinstance(spec, str):
        try:
            spec = tuple(int(x) for x in spec.lower().split("x"))
        except ValueError:
            spec = ()
    spec = tuple(int(x) for x in spec)
    if len(spec) != 3 or not (1 <= spec[0] <= len(PRUNE_L0) and 1 <= spec[1] <= len(PRUNE_L2_REL) and spec[2] >= 1):
        raise ValueError(f"prune_grid: expected N0xN2xN1 with N0 <= {len(PRUNE_L0)}, N2 <= {len(PRUNE_L2_REL)}, N1 >= 1")
    return spec


def prune_grid(mu: np.ndarray, S: np.ndarray, l0=PRUNE_L0, l2_rel=PRUNE_L2_REL, n1: int = 16) -> Dict:
    """The paths of ``prune_trees``, ``l0``-major over ``l0 x l2_rel``: ``b = mu + l0 mean(mu)``,
    ``l2 = l2_rel trace(S) / n``, ``l1 = max|b| 10^(-linspace(0, 3, n1))``."""
    n = mu.shape[0]
    if not len(l0) or not len(l2_rel) or int(n1) < 1:
        raise ValueError("tree prune: an empty penalty grid")
    b, l1s, l2, pen = [], [], [], []
    for a0 in l0:
        for r2 in l2_rel:
            bp = mu + float(a0) * mu.mean()
            b.append(bp)
            l2.append(float(r2) * np.trace(S) / n)
            l1s.append(np.abs(bp).max() * 10.0 ** (-np.linspace(0.0, 3.0, int(n1))))
            pen.append((float(a0), float(r2)))
    return {"b": np.array(b), "l1s": np.array(l1s), "l2": np.array(l2), "l0_l2_rel": pen}


def prune_trees(res_by_split: Dict, l0=PRUNE_L0, l2_rel=PRUNE_L2_REL, n1: int = 16, max_assets: int = 40,
                max_sweeps: int = 2000, device=None, depth_weight: bool = True) -> Dict:
    """Prune the tree nodes into a sparse mean-variance SDF. ``res_by_split``: the
    ``tree_sorted_portfolios`` results of the same trees on ``train``, ``valid`` and ``test``.

    The moments are the train split's (``node_returns``, ``mv_moments``; formed on the host), the paths
    ``prune_grid``'s, all on the one train ``S``, solved by ``en_paths`` on ``device``. A candidate
    ``theta`` gives the factor ``F[t] = R_split[t] . theta`` on every split and its ``sharpe_ddof0``. The
    selection is ``np.argmax`` of the validation Sharpe over the computed points with ``1 <= nnz <=
    max_assets`` (the first index wins a tie); there has to be one.

    Returns ``l0``, ``l2_rel``, ``l1``, ``l2`` and ``path``, ``point`` of the selection, its ``theta`` [n],
    ``nodes`` (a list of (tree, node, path, level, weight), the path as ``tree_sorts.node_path``), the
    Sharpe ratios ``train_sharpe``, ``valid_sharpe``, ``test_sharpe``, per candidate ([P][n1]) ``nnz``,
    ``sweeps``, ``computed``, ``eligible`` and ``sharpe`` (a dict of the three splits, NaN where not
    computed), the grid (``grid_l0``, ``grid_l2_rel``, ``grid_l1`` [P][n1], ``grid_l2`` [P]), ``assets``,
    ``max_assets``, ``depth_weight``, ``seconds`` and, from the kernel, ``gpu_ms`` and ``launches``."""
    missing = [s for s in SPLITS if s not in res_by_split]
    if missing:
        raise ValueError(f"tree prune: no tree sort for the split(s) {missing}")
    max_assets = int(max_assets)
    if max_assets < 1:
        raise ValueError("tree prune: max_assets must be at least 1")
    R, un = {}, None
    for s in SPLITS:
        R[s], u = node_returns(res_by_split[s], depth_weight)
        if un is not None and u["nodes"] != un["nodes"]:
            raise ValueError("tree prune: the splits were sorted on different trees")
        un = u
    mu, S = mv_moments(R["train"])
    grid = prune_grid(mu, S, l0, l2_rel, n1)
    P, n1 = grid["l1s"].shape
    t0 = time.perf_counter()
    sol = en_paths(S[None], np.zeros(P, np.int32), grid["b"], grid["l1s"], grid["l2"], max_sweeps=max_sweeps,
                   max_assets=max_assets, device="cpu" if device is None else device)
    seconds = time.perf_counter() - t0
    theta, nnz, sweeps = sol["theta"], sol["nnz"], sol["sweeps"]
    computed = sweeps > 0
    eligible = computed & (nnz >= 1) & (nnz <= max_assets)
    if not eligible.any():
        raise ValueError(f"tree prune: no computed point with 1 <= nnz <= {max_assets}")
    sharpe = {s: np.full((P, n1), np.nan) for s in SPLITS}
    for p, k in zip(*np.nonzero(computed)):
        for s in SPLITS:
            sharpe[s][p, k] = sharpe_ddof0(R[s] @ theta[p, k])
    sel = int(np.argmax(np.where(eligible, sharpe["valid"], -np.inf)))
    p, k = divmod(sel, n1)
    th = theta[p, k]
    res0 = res_by_split["train"]
    nodes = []
    lay = ts.tree_layout(res0["splits"])
    for a in np.flatnonzero(th):
        tr, nd = un["nodes"][a]
        lev = un["levels"][a]
        nodes.append((int(tr), int(nd), ts.node_path(res0["trees"][tr], lay["splits"], lev, nd - lay["level_offsets"][lev]),
                      int(lev), float(th[a])))
    a0, r2 = grid["l0_l2_rel"][p]
    out = {"l0": a0, "l2_rel": r2, "l1": float(grid["l1s"][p, k]), "l2": float(grid["l2"][p]), "path": int(p), "point": int(k),
           "theta": th.copy(), "nodes": nodes,
           "train_sharpe": float(sharpe["train"][p, k]), "valid_sharpe": float(sharpe["valid"][p, k]),
           "test_sharpe": float(sharpe["test"][p, k]),
           "nnz": nnz.copy(), "sweeps": sweeps.copy(), "computed": computed, "eligible": eligible, "sharpe": sharpe,
           "grid_l0": [float(x) for x in l0], "grid_l2_rel": [float(x) for x in l2_rel], "grid_l1": grid["l1s"],
           "grid_l2": grid["l2"], "assets": int(theta.shape[2]), "max_assets": max_assets,
           "depth_weight": bool(depth_weight), "names": list(res0["names"]), "seconds": float(seconds)}
    for key in ("gpu_ms", "launches"):
        if key in sol:
            out[key] = sol[key]
    return out


# ---- stock-level weights of the pruned SDF ---------------------------------------------------------
def node_coefficients(pr: Dict, res: Dict) -> np.ndarray:
    """``coef`` float64 [P][NN] of the pruned SDF ``pr`` on the trees of ``res``: ``theta[u] * (1 /
    sqrt(nodes_per_level[level_u]))`` (``node_returns``' own factor, one product; the factor is 1 without
    ``depth_weight``) at the representative (tree, node) of the distinct node ``u``, 0 everywhere else."""
    un = ts.unique_nodes(res["trees"], res["splits"])
    theta = np.asarray(pr["theta"], dtype=np.float64)
    if theta.shape != (len(un["nodes"]),):
        raise ValueError(f"tree prune: theta has {theta.shape} entries, the trees have {len(un['nodes'])} distinct nodes")
    lay = ts.tree_layout(res["splits"])
    fac = np.ones(theta.shape[0], np.float64)
    if pr.get("depth_weight", True):
        npl = np.asarray(lay["nodes_per_level"], dtype=np.float64)
        fac = 1.0 / np.sqrt(npl[np.asarray(un["levels"])])
    coef = np.zeros((len(res["trees"]), lay["nodes"]), np.float64)
    pi, ni = np.array([p for p, _ in un["nodes"]]), np.array([j for _, j in un["nodes"]])
    coef[pi, ni] = theta * fac
    return coef


def pruned_weights(pr: Dict, res_by_split: Dict, batches: Dict, models: Sequence, device: str = "cpu",
                   precision: str = "bf16", weights: Optional[Dict] = None) -> Dict:
    """The dense stock-level weight ``w`` float32 [T][N] (0 at the invalid cells) of the pruned SDF per
    split of ``res_by_split`` (``tree_sorted_portfolios`` results with their ``breaks``), on ``batches[split]``.
    By construction ``sum_i w[t, i] R[t, i] = R_split[t] . theta`` up to rounding; an empty node contributes
    a return of 0 and no stock weight. ``weights``: the ensemble weight per split, for trees that sort on
    it. ``device`` and ``precision`` have to be those of the sorts: the walk needs the sort's own keys."""
    out = {}
    for s, res in res_by_split.items():
        coef = node_coefficients(pr, res)
        out[s] = ts.tree_weights(models, batches[s], res, coef, device=device, precision=precision,
                                 weights=None if weights is None else weights.get(s))["w"]
    return out


def factor_from_weights(w: np.ndarray, returns, mask) -> np.ndarray:
    """``F[t] = sum_i w[t, i] R[t, i]`` over the valid cells in float64."""
    m = _host(mask, bool)
    return (np.asarray(w, dtype=np.float64) * _host(returns, np.float64) * m).sum(axis=1)


def pruned_metrics(pr: Dict, res_by_split: Dict, w_by_split: Dict, batches: Dict) -> Dict:
    """The paper's rows of the pruned SDF from its stock-level weights: ``paper_metrics`` of the test
    split on ``-w`` (that function's factor is ``-w . R``, the ensemble's sign), the three Sharpe ratios of
    ``sum_i w R`` and ``self_check``, the largest ``|sum_i w R - R_split . theta|`` over all periods."""
    from .portfolio import paper_metrics
    out, worst = {}, 0.0
    theta = np.asarray(pr["theta"], dtype=np.float64)
    for s in SPLITS:
        b = batches[s]
        f = factor_from_weights(w_by_split[s], b["returns"], b["mask"])
        ref = node_returns(res_by_split[s], pr.get("depth_weight", True))[0] @ theta
        worst = max(worst, float(np.abs(f - ref).max()) if f.size else 0.0)
        out[s + "_sharpe"] = sharpe_ddof0(f)
    tb = batches["test"]
    pm = paper_metrics(-np.asarray(w_by_split["test"], dtype=np.float32), _host(tb["returns"], np.float32), _host(tb["mask"], bool))
    out.update({k: pm[k] for k in ("ev", "xs_r2", "turnover", "max_1m_loss_std")})
    out["self_check"] = worst
    return out


def format_pruned_metrics(pm: Dict, gan: Optional[Dict] = None) -> List[str]:
    """The printed block of ``pruned_metrics`` (next to the ensemble's ``paper_metrics`` of the test split
    when the run has them)."""
    lines = [f"  {'':14s} {'EV':>8s} {'XS-R2':>8s} {'turnover':>9s} {'max 1m loss':>12s}",
             f"  {'Pruned trees':14s} {pm['ev']:8.4f} {pm['xs_r2']:8.4f} {pm['turnover']:9.3f} {pm['max_1m_loss_std']:9.2f} sd"]
    if gan is not None:
        lines.append(f"  {'Ensemble':14s} {gan['ev']:8.4f} {gan['xs_r2']:8.4f} {gan['turnover']:9.3f} {gan['max_1m_loss_std']:9.2f} sd")
    lines.append(f"  Sharpe from the stock-level weights:  train {pm['train_sharpe']:8.4f}  valid {pm['valid_sharpe']:8.4f}  "
                 f"test {pm['test_sharpe']:8.4f}")
    lines.append(f"  Self-check max |sum_i w R - R_split . theta| over all periods: {pm['self_check']:.3e}")
    return lines


def format_pruned(pr: Dict, gan: Optional[Dict] = None, key_names: Optional[Sequence] = None) -> List[str]:
    """The printed report: the selection, its Sharpe ratios (next to the ensemble's ``gan`` =
    {train_sharpe, valid_sharpe, test_sharpe} when given) and the selected nodes."""
    P, n1 = pr["nnz"].shape
    lines = [f"  {pr['assets']} assets, {P} paths x {n1} points ({int(pr['computed'].sum())} computed, "
             f"{int(pr['eligible'].sum())} with 1 <= nnz <= {pr['max_assets']})",
             f"  Selected: l0 {pr['l0']:g}  l2 {pr['l2_rel']:g} x tr(S)/n  l1 {pr['l1']:.3e}  (path {pr['path']}, point {pr['point']}): "
             f"{len(pr['nodes'])} nodes, {int(pr['sweeps'][pr['path'], pr['point']])} sweeps",
             f"  {'':14s} {'train':>8s} {'valid':>8s} {'test':>8s}",
             f"  {'Pruned trees':14s} {pr['train_sharpe']:8.4f} {pr['valid_sharpe']:8.4f} {pr['test_sharpe']:8.4f}"]
    if gan is not None:
        lines.append(f"  {'Ensemble':14s} {gan['train_sharpe']:8.4f} {gan['valid_sharpe']:8.4f} {gan['test_sharpe']:8.4f}")
    lines.append("  Nodes (key:child along the path, weight):")
    for tr, nd, path, lev, w in pr["nodes"]:
        name = " > ".join(f"{key_names[c] if key_names is not None else c}:{q}" for c, q in path) or "root"
        lines.append(f"    {w: .5e}  level {lev}  {name}")
    return lines


def pruned_to_json(pr: Dict) -> Dict:
    """Plain lists (non-finite values as null) of every key of ``prune_trees``' result."""
    out = {}
    for k, v in pr.items():
        if k == "nodes":
            out[k] = [{"tree": tr, "node": nd, "path": [[int(c), int(q)] for c, q in path], "level": lev, "weight": w}
                      for tr, nd, path, lev, w in v]
        elif k == "sharpe":
            out[k] = {s: _jsonable(a) for s, a in v.items()}
        elif isinstance(v, np.ndarray) and v.dtype == bool:
            out[k] = v.astype(int).tolist()
        else:
            out[k] = _jsonable(v)
    return out
