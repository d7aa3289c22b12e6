"""``k_encd`` (``tree_prune.en_paths`` on the GPU) against the numpy oracle: every comparison is on the
uint64 views of ``theta`` plus ``sweeps`` and ``nnz`` as integers, without a tolerance. The oracle of a
case is computed once (``prune_cases.oracle``)."""
import numpy as np
import pytest
import torch

import prune_cases as pc
from deeplearninginassetpricing_paperreplication_amd.analysis import tree_prune as tp

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _case(name):
    return pc.two_matrix_case() if name == "two_matrices" else pc.case(name)


def _run(c, rows=None, **kw):
    A, a_of, b, l1s, l2 = pc.call_args(c)
    if rows is not None:
        a_of, b, l1s, l2 = a_of[rows], b[rows], l1s[rows], l2[rows]
    return tp.en_paths(A, a_of, b, l1s, l2, max_sweeps=c["max_sweeps"], max_assets=c["max_assets"], device="cuda", **kw)


def _same(got, want, rows=None):
    sel = slice(None) if rows is None else rows
    assert got["theta"].dtype == np.float64 and got["sweeps"].dtype == np.int32 and got["nnz"].dtype == np.int32
    np.testing.assert_array_equal(got["sweeps"], want["sweeps"][sel])
    np.testing.assert_array_equal(got["nnz"], want["nnz"][sel])
    np.testing.assert_array_equal(_bits(got["theta"]), _bits(want["theta"][sel]))


# n = 1 .. 300: less than a wave, not a multiple of 64, more than one element per thread; then one case
# per row-buffer size of the kernel up to ENCD_MAX_N; l2 = 0 with T < n (the sweep cap), a zero diagonal,
# max_assets, two matrices through a_of
@pytest.mark.parametrize("name", ["n1", "n13", "n64", "n70", "n257", "n300", "n600", "n1100", "n2100", "n4096",
                                  "rank_deficient", "zero_diagonal", "max_assets", "two_matrices"])
def test_bits_of_the_oracle(name):
    got = _run(_case(name))
    want = pc.oracle(name)
    _same(got, want)
    assert got["launches"] >= 1 and len(got["launch_ms"]) == got["launches"] and got["gpu_ms"] > 0
    np.testing.assert_array_equal(got["path_updates"], want["updates"].sum(axis=1))


def test_native_limits():
    from deeplearninginassetpricing_paperreplication_amd.ops import native
    nat = native.load(required=True)
    assert nat.ENCD_MAX_N == 4096 and nat.encd_supported(1) and nat.encd_supported(4096)
    assert not nat.encd_supported(0) and not nat.encd_supported(4097)
    assert nat.encd_state_bytes(3, 70) == 3 * (2 * 70 * 8 + 16)
    assert nat.encd_threads() % 64 == 0


@pytest.mark.parametrize("name", ["n70", "n300"])
def test_a_path_alone_first_or_last(name):
    c, want = _case(name), pc.oracle(name)
    for rows in ([1], [1, 0, 2], [0, 2, 1], [2, 2, 1, 1]):
        _same(_run(c, rows=rows), want, rows)


@pytest.mark.parametrize("name", ["n70", "rank_deficient", "max_assets", "n1100"])
def test_sweeps_per_launch_changes_no_bit(name):
    c, want = _case(name), pc.oracle(name)
    most = int(want["sweeps"].sum(axis=1).max())
    for spl in (1, 7, None):
        got = _run(c, sweeps_per_launch=spl)
        _same(got, want)
        if spl is not None:                       # a launch runs at most spl sweeps of a path
            assert got["launches"] == -(-most // spl)


def test_inputs_on_the_device_are_not_written():
    c, want = _case("two_matrices"), pc.oracle("two_matrices")
    dev = torch.device("cuda", torch.cuda.current_device())
    A, a_of, b, l1s, l2 = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in pc.call_args(c))
    keep = [x.clone() for x in (A, a_of, b, l1s, l2)]
    ptrs = [x.data_ptr() for x in (A, b)]
    got = tp.en_paths(A, a_of, b, l1s, l2, max_sweeps=c["max_sweeps"], max_assets=c["max_assets"])
    _same(got, want)
    assert ptrs == [x.data_ptr() for x in (A, b)]
    for x, k in zip((A, a_of, b, l1s, l2), keep):
        assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, k.view(torch.int64) if k.dtype == torch.float64 else k)
    bad = A.clone(); bad[1, 3, 7] += 1.0
    with pytest.raises(ValueError, match="symmetric"):
        tp.en_paths(bad, a_of, b, l1s, l2)


def test_prune_trees_on_the_gpu_is_the_cpu_result():
    by_split = pc.planted_tree_results()
    kw = dict(n1=8, max_assets=6, max_sweeps=pc.MAX_SWEEPS)
    cpu = tp.prune_trees(by_split, device="cpu", **kw)
    gpu = tp.prune_trees(by_split, device="cuda", **kw)
    assert set(gpu) == set(cpu) | {"gpu_ms", "launches"} and gpu["gpu_ms"] > 0
    for k, v in cpu.items():
        if k == "seconds":
            continue
        if k == "sharpe":
            for s in tp.SPLITS:
                np.testing.assert_array_equal(_bits(gpu[k][s]), _bits(v[s]))
        elif isinstance(v, np.ndarray) and v.dtype == np.float64:
            np.testing.assert_array_equal(_bits(gpu[k]), _bits(v))
        elif isinstance(v, np.ndarray):
            np.testing.assert_array_equal(gpu[k], v)
        else:
            assert gpu[k] == v, k
