"""Tree-sorted portfolios priced by the SDF: sorts that condition on three or more keys at once (a
size x value x momentum ``2x3x3`` sort) and the asset-pricing trees of Bryzgalova, Pelger and Zhu
(repeated conditional median splits on a short list of characteristics, every intermediate and
final node a portfolio).

Definition (one rule, applied per level; ``tree_sort_numpy`` is the oracle, ``Engine.tree_sorted_portfolios``
/ ``csrc/k_qtree.hip`` the GPU path). A call takes ``splits = (Q_1, .., Q_D)`` with every ``Q_l`` in
``2..16`` and ``L = prod Q_l <= 36`` leaves (so ``D <= 5``), and ``P`` trees, each a sequence
``(c_1, .., c_D)`` of key indices (a key may repeat). For a period with ``n`` valid rows:

* Level 0 has one node, the root, with all ``n`` rows. Level ``l >= 1`` has ``n_l = Q_1 .. Q_l`` nodes.
* A node ``a`` of level ``l - 1`` holds ``m_a`` rows. With ``s`` those rows' ``c_l`` keys ascending
  (``-0.0`` equals ``+0.0``) its breakpoints are ``b_{a,d} = s[ceil(d m_a / Q_l) - 1]``, ``d = 1..Q_l-1``,
  and a row of the node goes to child ``q = #{ d : key > b_{a,d} }``, node ``a Q_l + q`` of level ``l``.
* Tied keys share the lowest child any of them would get. ``m_a = 0`` leaves the node's breakpoints
  NaN and its subtree empty, ``m_a < Q_l`` leaves some children empty; an empty period gives zero
  counts and sums and NaN breakpoints.
* ``D = 1`` is the single sort (``sorted_portfolios.sort_buckets_numpy``), ``D = 2`` the conditional
  double sort (``double_sort_numpy``). There is no independent mode.

Layout, level order (``tree_layout``): ``off[l] = n_0 + .. + n_{l-1}``, node ``(l, j)`` at ``off[l] + j``
(the root is node 0), ``NN = off[D+1]`` nodes; ``boff[l] = sum_{k<l} n_k (Q_{k+1} - 1)``, breakpoint
``(l, a, d)`` at ``boff[l-1] + a (Q_l - 1) + (d - 1)``, ``NB = boff[D] = L - 1`` breakpoints.

Per (period, tree, node) the raw result holds the row count and the float64 sums of the value
columns (the return, then the ensemble weight); per (period, tree) ``breaks`` [NB].

Pruning the nodes into an SDF (the elastic-net mean-variance step of the tree paper) is
``analysis.tree_prune``. A combination of nodes is also a weight per stock-month, since a node is an
equally weighted basket: ``tree_weights_numpy`` is its definition, ``tree_weights`` runs it on the CPU or
through ``Engine.tree_weights`` / ``csrc/k_qtree_weight.hip`` with the same bits.

Out of scope: sharing selects between trees with a common prefix, an independent (non-nested) mode, value
weighting beyond a caller's value column, more than 36 leaves, plots.
"""
from __future__ import annotations

import itertools
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import sorted_portfolios as sp

MAX_Q = sp.MAX_Q
MAX_LEAVES = 36
MAX_DEPTH = 5
MAX_TREES = 4096


def _check_splits(splits) -> tuple:
    try:
        qs = tuple(int(q) for q in splits)
    except (TypeError, ValueError):
        raise ValueError("splits must be a sequence (Q_1, .., Q_D) of integers") from None
    if not 1 <= len(qs) <= MAX_DEPTH:
        raise ValueError(f"splits must have 1 to {MAX_DEPTH} levels")
    if any(q < 2 or q > MAX_Q for q in qs):
        raise ValueError(f"every split must be in [2, {MAX_Q}]")
    if int(np.prod(qs)) > MAX_LEAVES:
        raise ValueError(f"the product of the splits must be at most {MAX_LEAVES}")
    return qs


def parse_tree_splits(spec, depth: Optional[int] = None) -> tuple:
    """``splits`` from one integer (every level of a tree of ``depth``), the CLI form ``"2x3x3"`` or a
    sequence; checked, and against ``depth`` when given."""
    if isinstance(spec, str):
        try:
            qs = [int(x) for x in spec.lower().split("x")]
        except ValueError:
            raise ValueError(f"tree_splits: expected Q or Q1xQ2x.., got {spec!r}") from None
        spec = qs[0] if len(qs) == 1 else qs
    if isinstance(spec, (int, np.integer)):
        if depth is None:
            raise ValueError("tree_splits: one integer needs the depth of the trees")
        spec = (int(spec),) * int(depth)
    qs = _check_splits(spec)
    if depth is not None and len(qs) != int(depth):
        raise ValueError(f"tree_splits: {len(qs)} levels for trees of depth {depth}")
    return qs


def tree_layout(splits) -> Dict:
    """The node and breakpoint layout of ``splits``: ``nodes_per_level`` [D+1], ``level_offsets`` [D+2],
    ``break_offsets`` [D+1], ``nodes`` (NN), ``breaks`` (NB), ``leaves`` (L), ``depth`` and ``splits``."""
    qs = _check_splits(splits)
    n, off, boff = [1], [0, 1], [0]
    for q in qs:
        boff.append(boff[-1] + n[-1] * (q - 1))
        n.append(n[-1] * q)
        off.append(off[-1] + n[-1])
    return {"splits": qs, "depth": len(qs), "nodes_per_level": n, "level_offsets": off, "break_offsets": boff,
            "nodes": off[-1], "breaks": boff[-1], "leaves": n[-1]}


def _check_trees(trees: Sequence, depth: int, n_keys: int) -> List[tuple]:
    out = []
    for tr in trees:
        try:
            tr = tuple(int(c) for c in tr)
        except (TypeError, ValueError):
            raise ValueError(f"tree sorts: expected a sequence of key indices, got {tr!r}") from None
        if len(tr) != depth:
            raise ValueError(f"tree sorts: tree {tr!r} has {len(tr)} keys, splits has {depth} levels")
        if any(c < 0 or c >= n_keys for c in tr):
            raise ValueError(f"tree sorts: tree {tr!r} outside the {n_keys} key columns")
        out.append(tr)
    if len(out) > MAX_TREES:
        raise ValueError(f"tree sorts: at most {MAX_TREES} trees per call, got {len(out)}")
    return out


def tree_sort_numpy(keys: np.ndarray, trees: Sequence, mask: np.ndarray, values: np.ndarray, splits) -> Dict:
    """The definition in numpy. ``keys`` [T][N][P'] (float32 or float64), ``trees`` a list of
    sequences of D columns of ``keys``, ``mask`` [T][N], ``values`` [T][N][V]. Returns ``count`` int32
    [T][P][NN], ``sum`` float64 [T][P][NN][V] (every node summed over its own rows), ``breaks``
    [T][P][NB] in the keys' dtype (NaN where the period or the node is empty), ``level_offsets``,
    ``break_offsets`` and ``rows``."""
    lay = tree_layout(splits)
    qs, D, off, boff, nl = lay["splits"], lay["depth"], lay["level_offsets"], lay["break_offsets"], lay["nodes_per_level"]
    keys = np.asarray(keys)
    mask = np.asarray(mask).astype(bool)
    values = np.asarray(values)
    T, N, PK = keys.shape
    V = values.shape[2]
    trees = _check_trees(trees, D, PK)
    P = len(trees)
    count = np.zeros((T, P, lay["nodes"]), np.int32)
    sums = np.zeros((T, P, lay["nodes"], V), np.float64)
    breaks = np.full((T, P, lay["breaks"]), np.nan, keys.dtype)
    zero = keys.dtype.type(0)
    for t in range(T):
        idx = np.nonzero(mask[t])[0]
        n = int(idx.size)
        if n == 0:
            continue
        v = values[t, idx, :].astype(np.float64)
        for p, tr in enumerate(trees):
            node = np.zeros(n, np.int64)
            count[t, p, 0] = n
            sums[t, p, 0] = v.sum(axis=0)
            for l in range(1, D + 1):
                Q = qs[l - 1]
                k = keys[t, idx, tr[l - 1]] + zero               # (-0.0 + 0.0 = +0.0)
                child = np.zeros(n, np.int64)
                for a in range(nl[l - 1]):
                    sel = node == a
                    if not sel.any():
                        continue
                    b = sp._breaks(np.sort(k[sel]), Q)
                    breaks[t, p, boff[l - 1] + a * (Q - 1):boff[l - 1] + (a + 1) * (Q - 1)] = b
                    child[sel] = a * Q + (k[sel][:, None] > b[None, :]).sum(axis=1)
                node = child
                onehot = (node[None, :] == np.arange(nl[l])[:, None]).astype(np.float64)    # [nodes][n]
                count[t, p, off[l]:off[l + 1]] = onehot.sum(axis=1).astype(np.int32)
                sums[t, p, off[l]:off[l + 1]] = onehot @ v
    return {"count": count, "sum": sums, "breaks": breaks, "level_offsets": list(off), "break_offsets": list(boff),
            "rows": int(mask.sum())}


def all_trees(keys: Sequence, depth: int) -> List[tuple]:
    """Every ordered sequence of ``depth`` members of ``keys`` with repetition (the asset-pricing-tree
    set: 3 characteristics at depth 4 give 81 trees of 31 nodes)."""
    keys = list(keys)
    depth = int(depth)
    if not keys or not 1 <= depth <= MAX_DEPTH:
        raise ValueError(f"all_trees: needs at least one key and a depth in [1, {MAX_DEPTH}]")
    if len(keys) ** depth > MAX_TREES:
        raise ValueError(f"tree sorts: at most {MAX_TREES} trees per call, got {len(keys) ** depth}")
    return list(itertools.product(keys, repeat=depth))


def node_path(tree: Sequence, splits: Sequence, level: int, j: int) -> tuple:
    """The path ``((c_1, q_1), .., (c_l, q_l))`` of node ``j`` of level ``level``."""
    qs = []
    for l in range(level, 0, -1):
        j, q = divmod(j, int(splits[l - 1]))
        qs.append(q)
    return tuple((tree[l], q) for l, q in enumerate(reversed(qs)))


def unique_nodes(trees: Sequence, splits) -> Dict:
    """The distinct portfolios among the nodes of ``trees``: two nodes of different trees are the
    same portfolio exactly when their paths ``((c_1, q_1), .., (c_l, q_l))`` are equal. One
    representative is kept per path (the first in tree, then node, order) and the root once.
    Returns ``nodes`` and ``leaves`` (the representatives of depth D), lists of (tree, node index),
    and ``levels``, the level of every entry of ``nodes``."""
    lay = tree_layout(splits)
    qs, D, off, nl = lay["splits"], lay["depth"], lay["level_offsets"], lay["nodes_per_level"]
    seen, nodes, levels = set(), [], []
    for p, tr in enumerate(trees):
        tr = tuple(tr)
        if len(tr) != D:
            raise ValueError(f"tree sorts: tree {tr!r} has {len(tr)} keys, splits has {D} levels")
        for l in range(D + 1):
            for j in range(nl[l]):
                path = node_path(tr, qs, l, j)
                if path in seen:
                    continue
                seen.add(path)
                nodes.append((p, off[l] + j))
                levels.append(l)
    return {"nodes": nodes, "levels": levels, "leaves": [nd for nd, l in zip(nodes, levels) if l == D]}


def _resolve_trees(trees: Sequence, F: int, names: Optional[Sequence]) -> List[tuple]:
    """Tree members as key indices: a column in [0, F), or ``F`` / ``"weight"`` for the ensemble
    weight (a characteristic's name when ``names`` is given)."""
    idx = {str(nm): i for i, nm in enumerate(names)} if names is not None and len(names) == F else {}

    def one(m):
        if isinstance(m, str):
            m = m.strip()
            if m == "weight":
                return F
            if m in idx:
                return idx[m]
            try:
                m = int(m)
            except ValueError:
                raise ValueError(f"tree sorts: unknown key {m!r}") from None
        m = int(m)
        if m < 0 or m > F:
            raise ValueError(f"tree sorts: key {m} outside [0, {F}] ({F} is the weight)")
        return m
    out = []
    for tr in trees:
        if isinstance(tr, (str, int, np.integer)):
            raise ValueError(f"tree sorts: expected a sequence of keys, got {tr!r}")
        out.append(tuple(one(m) for m in tr))
    return out


def parse_trees(spec) -> List:
    """CLI form of ``trees``: a comma list of ``A:B:C`` by name, column index or ``weight``
    (anything else is returned as it is)."""
    if not isinstance(spec, str):
        return list(spec)
    return [tuple(tok.strip() for tok in item.split(":")) for item in spec.split(",") if item.strip()]


def _gpu_raw(spec, batch, w: torch.Tensor, trees, splits, precision: str) -> Dict:
    from ..engine.runner import GANEngine
    eng = GANEngine(spec, 1, max_epochs=4, precision=precision)
    eng.set_data(batch)
    torch.cuda.synchronize(w.device)
    try:
        r = eng.eng.tree_sorted_portfolios(0, [list(tr) for tr in trees], list(splits), w.data_ptr(), 1, w.data_ptr(), 1)
    finally:
        eng.eng.sync()
    out = {k: np.asarray(r[k]) for k in ("count", "sum", "breaks")}
    out["gpu_ms"] = float(r["gpu_ms"])
    return out


def tree_sorted_portfolios(models: Sequence, batch: Dict, trees: Sequence, splits=None, device: str = "cpu",
                           names: Optional[Sequence] = None, weights: Optional[np.ndarray] = None,
                           precision: str = "bf16") -> Dict:
    """Equally weighted tree-sorted portfolios of ``batch`` for every tree of ``trees``: members are
    column indices (or names, with ``names``), or ``F`` / ``"weight"`` for the ensemble weight (on the
    GPU the weight is the engine method's one extra key). ``splits``: ``(Q_1, .., Q_D)``, default a
    median split at every level of the trees.

    Returns ``returns`` and ``loading`` [T][P][NN] (node mean return / ensemble weight, NaN where the
    node is empty), ``count`` int32 [T][P][NN], ``breaks`` [T][P][NB], ``trees`` (resolved indices),
    ``names`` (``"A > B > C"``), ``splits``, ``level_offsets``, ``break_offsets`` and, on the GPU,
    ``gpu_ms``. ``weights`` and ``precision`` as for ``sorted_portfolios.sorted_portfolios``."""
    models = list(models)
    mask = batch["mask"].bool()
    T, N, F = batch["individual_features"].shape
    trs = _resolve_trees(trees, F, names)
    if splits is None:
        if not trs:
            raise ValueError("tree sorts: splits is needed with an empty tree list")
        splits = (2,) * len(trs[0])
    lay = tree_layout(splits)
    trs = _check_trees(trs, lay["depth"], F + 1)
    gpu = str(device).startswith("cuda")
    if gpu:
        from ..ops import native
        if native.load(required=False) is None:
            print("[tree_sorts] native extension not available: using the CPU path")
            gpu = False
    if not models and (weights is None or gpu):      # (the engine is built from a model's spec)
        raise ValueError("no models")
    if gpu:
        dev = torch.device("cuda", torch.cuda.current_device())
        if weights is None:
            w = sp._gpu_weights(models, batch)
        else:
            w = torch.as_tensor(np.asarray(weights, dtype=np.float32)).to(dev).contiguous()
        raw = _gpu_raw(models[0].spec, batch, w, trs, lay["splits"], precision)
    else:
        cpu = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
        w = sp._cpu_weights(models, cpu) if weights is None else np.asarray(weights)
        w = w.astype(np.float32)
        keys = np.concatenate([cpu["individual_features"].numpy().astype(np.float32), w[:, :, None]], axis=2)
        vals = np.stack([cpu["returns"].numpy().astype(np.float32), w], axis=2)
        raw = tree_sort_numpy(keys, trs, mask.cpu().numpy(), vals, lay["splits"])
    cnt = raw["count"]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(cnt[..., None] > 0, raw["sum"] / cnt[..., None], np.nan)
    kn = sp._key_names(F, True, names)
    out = {"returns": mean[..., 0], "loading": mean[..., 1], "count": cnt, "breaks": raw["breaks"], "trees": trs,
           "names": [" > ".join(kn[c] for c in tr) for tr in trs], "splits": lay["splits"],
           "level_offsets": list(lay["level_offsets"]), "break_offsets": list(lay["break_offsets"])}
    if "gpu_ms" in raw:
        out["gpu_ms"] = raw["gpu_ms"]
    return out


# ---- stock-level weights of a combination of nodes ---------------------------------------------------
MAX_WEIGHT_KEYS = 32      # distinct key columns of a GPU call (QTREE_WEIGHT_MAX_KEYS of csrc/qtree_weight.h)


def _check_coef(coef, P: int, NN: int) -> np.ndarray:
    coef = np.ascontiguousarray(np.asarray(coef), dtype=np.float64)
    if coef.shape != (P, NN):
        raise ValueError(f"tree weights: coef must be [{P}][{NN}] (trees x nodes), got {list(coef.shape)}")
    if not np.isfinite(coef).all():
        raise ValueError("tree weights: coef must be finite")
    return coef


def active_keys(trees: Sequence, splits, coef: np.ndarray) -> List[int]:
    """The distinct key columns a weight pass reads: those of the levels ``1 .. deepest level with a
    non-zero coefficient`` of every tree, in the order of first use."""
    off = tree_layout(splits)["level_offsets"]
    out: List[int] = []
    for p, tr in enumerate(trees):
        lv = [l for l in range(len(off) - 1) if np.any(np.asarray(coef)[p, off[l]:off[l + 1]] != 0)]
        for c in tr[:max(lv) if lv else 0]:
            if c not in out:
                out.append(int(c))
    return out


def _active_depths(splits, coef: np.ndarray) -> List[int]:
    """Per tree the deepest level with a non-zero coefficient (-1: none)."""
    off = tree_layout(splits)["level_offsets"]
    return [max([l for l in range(len(off) - 1) if np.any(coef[p, off[l]:off[l + 1]] != 0)], default=-1)
            for p in range(coef.shape[0])]


def tree_weights_numpy(keys: np.ndarray, trees: Sequence, mask: np.ndarray, splits, breaks: np.ndarray, count: np.ndarray,
                       coef: np.ndarray, dtype=np.float32) -> np.ndarray:
    """The stock-level weight of a combination of tree nodes: the definition in numpy. A node is an
    equally weighted basket, so ``coef`` float64 [P][NN] (finite, ``-0.0`` read as 0) over the nodes of
    the ``P`` trees is a weight per stock-month. ``keys`` [T][N][P'], ``trees``, ``mask``, ``splits`` as for
    ``tree_sort_numpy``; ``breaks`` [T][P][NB] and ``count`` [T][P][NN] of a tree sort of these keys.

    A valid row ``(t, i)`` follows the sort's rule down every tree, ``node_0 = 0``, ``node_l = node_{l-1} Q_l +
    #{d : key_{c_l} + 0 > b_{node_{l-1}, d}}`` (a comparison with a NaN breakpoint is false), and collects ::

        acc = +0.0 (float64)
        for p ascending, for l = 0 .. D ascending, j = level_offsets[l] + node_l:
            if coef[p][j] != 0:  acc = acc + coef[p][j] / count[t][p][j]      one division, one addition
        w[t, i] = dtype(acc)

    Returns ``w`` [T][N] in ``dtype`` (float32, or float64 for the unrounded ``acc``), 0 at the invalid
    cells. A visited node with a non-zero coefficient and ``count == 0`` means the breakpoints are not
    those of these keys: ``ValueError``."""
    lay = tree_layout(splits)
    qs, D, off, boff, nl = lay["splits"], lay["depth"], lay["level_offsets"], lay["break_offsets"], lay["nodes_per_level"]
    keys = np.asarray(keys)
    mask = np.asarray(mask).astype(bool)
    T, N, PK = keys.shape
    trees = _check_trees(trees, D, PK)
    P = len(trees)
    breaks, count = np.asarray(breaks), np.asarray(count)
    if breaks.shape != (T, P, lay["breaks"]) or count.shape != (T, P, lay["nodes"]):
        raise ValueError("tree weights: breaks must be [T][P][NB] and count [T][P][NN] of a tree sort of these trees")
    coef = _check_coef(coef, P, lay["nodes"])
    if np.dtype(dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("tree weights: dtype must be float32 or float64")
    zero = keys.dtype.type(0)
    depth = _active_depths(splits, coef)
    out = np.zeros((T, N), np.float64)
    for t in range(T):
        idx = np.nonzero(mask[t])[0]
        n = int(idx.size)
        if n == 0:
            continue
        acc = np.zeros(n, np.float64)
        for p, tr in enumerate(trees):
            node = np.zeros(n, np.int64)
            for l in range(depth[p] + 1):           # (the levels below add nothing: their coefficients are 0)
                if l >= 1:
                    Q = qs[l - 1]
                    k = keys[t, idx, tr[l - 1]] + zero                  # (-0.0 + 0.0 = +0.0)
                    b = breaks[t, p, boff[l - 1]:boff[l]].reshape(nl[l - 1], Q - 1)
                    node = node * Q + (k[:, None] > b[node]).sum(axis=1)
                c = coef[p, off[l] + node]
                nz = c != 0
                if nz.any():
                    m = count[t, p, off[l] + node[nz]]
                    if (m <= 0).any():
                        raise ValueError(f"tree weights: a row of period {t} reaches an empty node of tree {p} (level {l}): "
                                         "the breakpoints are not those of these keys")
                    acc[nz] = acc[nz] + c[nz] / m.astype(np.float64)
        out[t, idx] = acc
    return out.astype(dtype)


def _gpu_tree_weights(spec, batch, w: Optional[torch.Tensor], trees, splits, breaks, count, coef, precision: str,
                      want_acc: bool, trees_per_pass: Optional[int]) -> Dict:
    from ..engine.runner import GANEngine
    eng = GANEngine(spec, 1, max_epochs=4, precision=precision)
    eng.set_data(batch)
    dev = torch.device("cuda", torch.cuda.current_device())
    T, N = batch["mask"].shape
    w_out = torch.zeros((T, N), dtype=torch.float32, device=dev)
    acc_out = torch.zeros((T, N), dtype=torch.float64, device=dev) if want_acc else None
    torch.cuda.synchronize(dev)
    try:
        # a level below a tree's deepest non-zero one is never read: its key is handed over as column 0, so
        # that a tree that names the weight only there needs no extra key
        depth = _active_depths(splits, coef)
        trees = [[c if l < depth[p] else 0 for l, c in enumerate(tr)] for p, tr in enumerate(trees)]
        r = eng.eng.tree_weights(0, trees, list(splits), np.ascontiguousarray(breaks, dtype=np.float32),
                                 np.ascontiguousarray(count, dtype=np.int32), coef, 0 if w is None else w.data_ptr(),
                                 0 if w is None else 1, w_out.data_ptr(), 0 if acc_out is None else acc_out.data_ptr(),
                                 int(trees_per_pass or 0))
    finally:
        eng.eng.sync()
    out = {"w": w_out.cpu().numpy(), "gpu_ms": float(r["gpu_ms"]), "active_trees": int(r["active_trees"]),
           "passes": int(r["passes"])}
    if acc_out is not None:
        out["acc"] = acc_out.cpu().numpy()
    return out


def tree_weights(models: Sequence, batch: Dict, res: Dict, coef: np.ndarray, device: str = "cpu",
                 names: Optional[Sequence] = None, weights: Optional[np.ndarray] = None, precision: str = "bf16",
                 acc: bool = False, trees_per_pass: Optional[int] = None) -> Dict:
    """The stock-level weight of ``sum_nodes coef[p][j] x (node (p, j) of res)``: ``res`` a
    ``tree_sorted_portfolios`` result of ``batch`` (its ``trees``, ``splits``, ``breaks`` and ``count`` are read),
    ``coef`` float64 [P][NN]. On the CPU it is ``tree_weights_numpy`` on the float32 keys; on the GPU
    ``Engine.tree_weights`` (``csrc/k_qtree_weight.hip``) on an engine built as the sort's, with the
    ensemble weight as the one extra key when a level that is read uses ``weight`` (a tree's levels below
    its deepest non-zero coefficient are not read, and a tree that names ``weight`` only there needs none).
    ``models``, ``weights`` and ``precision`` as for ``tree_sorted_portfolios`` (neither is needed on the CPU when
    no level that is read uses the weight). Outside ``qtree_weight_supported`` the GPU call runs numpy on the
    keys the engine would hold (characteristics rounded to bf16 for ``precision="bf16"``) and says so.

    Returns ``w`` float32 [T][N] (0 at the invalid cells), with ``acc=True`` also ``acc`` float64, and from
    the kernel ``gpu_ms``, ``active_trees`` and ``passes``. No output bit depends on ``trees_per_pass``."""
    models = list(models)
    mask = batch["mask"].bool()
    T, N, F = batch["individual_features"].shape
    lay = tree_layout(res["splits"])
    trs = _check_trees(_resolve_trees(res["trees"], F, names), lay["depth"], F + 1)
    coef = _check_coef(coef, len(trs), lay["nodes"])
    breaks, count = np.asarray(res["breaks"]), np.asarray(res["count"])
    used = active_keys(trs, lay["splits"], coef)
    need_w = F in used
    gpu = str(device).startswith("cuda")
    engine_keys = False                                          # numpy on the keys an engine of ``precision`` holds
    if gpu:
        from ..ops import native
        nat = native.load(required=False)
        if nat is None:
            print("[tree_weights] native extension not available: using the CPU path")
            gpu = False
        elif not nat.qtree_weight_supported(list(lay["splits"]), len(trs), int(T), len(used)):
            print(f"[tree_weights] {len(used)} distinct keys, {len(trs)} trees, {int(T)} periods are outside "
                  f"qtree_weight_supported (at most {nat.QTREE_WEIGHT_MAX_KEYS} keys, {nat.QTREE_WEIGHT_MAX_TREES} trees, "
                  "65535 periods): using the numpy path")
            gpu, engine_keys = False, True
    if not models and (gpu or (need_w and weights is None)):     # (the engine is built from a model's spec)
        raise ValueError("no models")
    if gpu:
        dev = torch.device("cuda", torch.cuda.current_device())
        w = None
        if need_w:
            w = (sp._gpu_weights(models, batch) if weights is None
                 else torch.as_tensor(np.asarray(weights, dtype=np.float32)).to(dev).contiguous())
        out = _gpu_tree_weights(models[0].spec, batch, w, trs, lay["splits"], breaks, count, coef, precision, acc,
                                trees_per_pass)
        if not np.isfinite(out["w"]).all():
            raise ValueError("tree weights: a row reaches an empty node with a non-zero coefficient (or the weight leaves "
                             "float32): the breakpoints are not those of these keys")
        return out
    cpu = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    feats = cpu["individual_features"]
    if engine_keys and precision == "bf16":                      # (res was sorted on the engine's bf16 panel)
        feats = feats.to(torch.bfloat16).to(torch.float32)
    keys = feats.numpy().astype(np.float32)
    if need_w:
        w = sp._cpu_weights(models, cpu) if weights is None else np.asarray(weights)
        wk = w.astype(np.float32)[:, :, None]
    else:
        wk = np.zeros((T, N, 1), np.float32)
    keys = np.concatenate([keys, wk], axis=2)
    a64 = tree_weights_numpy(keys, trs, mask.cpu().numpy(), lay["splits"], breaks, count, coef, dtype=np.float64)
    out = {"w": a64.astype(np.float32)}
    if acc:
        out["acc"] = a64
    return out


def _subset(res: Dict, nodes: Sequence) -> Dict:
    """The (tree, node) entries ``nodes`` of ``res`` as one key with ``len(nodes)`` buckets."""
    pi, ni = np.array([p for p, _ in nodes]), np.array([j for _, j in nodes])
    return {"names": ["nodes"], **{k: np.asarray(res[k])[:, pi, ni][:, None, :] for k in ("count", "returns", "loading")}}


def price_tree_sorted(res: Dict, weights: np.ndarray, returns: np.ndarray, mask: np.ndarray) -> Dict:
    """Price the ``P * NN`` test assets of ``res`` (``tree_sorted_portfolios``) with the SDF weight
    ``weights`` [T][N], by ``sorted_portfolios.price_portfolios`` with the nodes as the buckets.

    Per node ([P][NN]): ``mean_ret``, ``alpha``, ``t_alpha``, ``ev_asset``. Per tree ([P], over its
    non-root nodes that exist, the formulas of ``price_portfolios``' overall numbers): ``tree_ev``,
    ``tree_xs_r2``, ``tree_mean_abs_alpha``, and the last-leaf-minus-first-leaf spread over the periods
    where both exist, ``hml`` with its Sharpe ratio ``hml_sharpe``. Over the unique nodes of all trees
    (``unique_nodes``: a node shared by several trees counts once): ``ev``, ``xs_r2``,
    ``mean_abs_alpha``, ``assets``; the same three over the unique leaves: ``leaves_ev``,
    ``leaves_xs_r2``, ``leaves_mean_abs_alpha``, with ``leaves`` their number."""
    cnt = np.asarray(res["count"])
    T, P, NN = cnt.shape
    if P == 0:
        raise ValueError("tree sorts: no trees to price")
    lay = tree_layout(res["splits"])
    first, last = lay["level_offsets"][lay["depth"]], NN - 1

    def part(psel, nsel):
        return {"names": list(res["names"])[psel],
                **{k: np.asarray(res[k])[:, psel][:, :, nsel] for k in ("count", "returns", "loading")}}
    allp = sp.price_portfolios(part(slice(None), slice(None)), weights, returns, mask)
    out = {k: allp[k] for k in ("mean_ret", "alpha", "t_alpha", "ev_asset")}
    per = [sp.price_portfolios(part(slice(p, p + 1), slice(1, None)), weights, returns, mask) for p in range(P)]
    ends = sp.price_portfolios(part(slice(None), [first, last]), weights, returns, mask)
    un = unique_nodes(res["trees"], res["splits"])
    pu = sp.price_portfolios(_subset(res, un["nodes"]), weights, returns, mask)
    pl = sp.price_portfolios(_subset(res, un["leaves"]), weights, returns, mask)
    out.update({"tree_ev": np.array([q["ev"] for q in per], np.float64),
                "tree_xs_r2": np.array([q["xs_r2"] for q in per], np.float64),
                "tree_mean_abs_alpha": np.array([q["mean_abs_alpha"] for q in per], np.float64),
                "hml": ends["hml"], "hml_sharpe": ends["hml_sharpe"],
                "ev": pu["ev"], "xs_r2": pu["xs_r2"], "mean_abs_alpha": pu["mean_abs_alpha"], "assets": pu["assets"],
                "leaves_ev": pl["ev"], "leaves_xs_r2": pl["xs_r2"], "leaves_mean_abs_alpha": pl["mean_abs_alpha"],
                "leaves": pl["assets"], "unique_nodes": len(un["nodes"]), "names": list(res["names"]),
                "splits": tuple(res["splits"]), "level_offsets": list(lay["level_offsets"])})
    return out


def format_tree_sorted(priced: Dict, top: int = 10) -> List[str]:
    """The printed report: the overall lines (unique nodes, unique leaves), then per tree (all of
    them up to ``top``, else the ``top`` with the largest last-minus-first-leaf spread) its EV /
    XS-R2 / mean |alpha| over its non-root nodes, the spread with its Sharpe ratio, and the leaves'
    mean returns."""
    P, NN = priced["mean_ret"].shape
    first = priced["level_offsets"][-2]
    sx = "x".join(str(q) for q in priced["splits"])
    lines = [f"  {priced['assets']} test assets ({P} trees x {NN} nodes, splits {sx}, {priced['unique_nodes']} distinct):  "
             f"EV {priced['ev']:7.4f}  XS-R2 {priced['xs_r2']:7.4f}  mean |alpha| {priced['mean_abs_alpha']:.3e}",
             f"  {priced['leaves']} distinct leaves:  EV {priced['leaves_ev']:7.4f}  XS-R2 {priced['leaves_xs_r2']:7.4f}  "
             f"mean |alpha| {priced['leaves_mean_abs_alpha']:.3e}"]
    order = np.arange(P)
    if P > top:
        h = np.nan_to_num(np.abs(priced["hml"]), nan=-1.0)
        order = np.argsort(-h, kind="stable")[:top]
        lines.append(f"  Top {top} trees by |last leaf - first leaf|:")
    for p in order:
        lines.append(f"  {priced['names'][p]}:  EV {priced['tree_ev'][p]:7.4f}  XS-R2 {priced['tree_xs_r2'][p]:7.4f}  "
                     f"mean |alpha| {priced['tree_mean_abs_alpha'][p]:.3e}  H-L {priced['hml'][p]: .4f}  "
                     f"SR {priced['hml_sharpe'][p]: .3f}")
        lines.append("    " + " ".join(f"{v: .4f}" for v in priced["mean_ret"][p][first:]))
    return lines


def tree_to_json(res: Dict, priced: Optional[Dict] = None) -> Dict:
    """Plain lists (non-finite values as null): the counts of ``res`` summed over the periods, the
    layout and every key of ``priced``."""
    out = {"names": list(res["names"]), "trees": [list(tr) for tr in res["trees"]],
           "splits": [int(q) for q in res["splits"]], "level_offsets": [int(o) for o in res["level_offsets"]],
           "break_offsets": [int(o) for o in res["break_offsets"]], "periods": int(res["count"].shape[0]),
           "count": sp._jsonable(res["count"].sum(axis=0))}
    if priced is not None:
        out.update({k: sp._jsonable(v) for k, v in priced.items()})
    return out
