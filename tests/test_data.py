"""Data layer vs the reference loader (the reference's ``src/data_loader.py``) on the shipped
synthetic panel, plus the engine's compacted split layout. The reference loader's tensors are
recorded as digests in ``tests/golden/data_loader.*`` (bit equality, ``tools/record_golden.py``)."""
import os

import numpy as np
import pytest
import torch

import golden_cases as gc
from deeplearninginassetpricing_paperreplication_amd.data.dataset import (
    AssetPricingDataset, create_data_loaders, create_small_sample, load_splits)
from deeplearninginassetpricing_paperreplication_amd.engine.panel import (
    bf16_bits_to_f32, f32_to_bf16_bits, prepare_split)

_paths = gc.shipped_paths


@pytest.fixture(scope="module")
def golden():
    return gc.load_json("data_loader.json"), gc.load_npz("data_loader.npz")


def test_dataset_matches_reference(golden, shipped_data):
    want, arrs = golden
    c, m = _paths(shipped_data, "train")
    b = AssetPricingDataset(c, m)
    ba, bb = want["train_full_batch"], b.get_full_batch()
    assert set(ba) == set(bb)
    for k in ba:
        assert ba[k]["dtype"] == str(bb[k].dtype), k
        assert ba[k]["digest"] == gc.digest(bb[k]), k
    for x, y in zip((arrs["macro_mean"], arrs["macro_std"]), b.get_macro_stats()):
        np.testing.assert_array_equal(x, y)
    assert want["train_len"] == len(b)
    for i in (0, 7, len(b) - 1):
        ia, ib = want["train_items"][str(i)], b[i]
        assert set(ia) == set(ib)
        for k in ia:
            assert ia[k] == gc.digest(torch.as_tensor(ib[k])), k


def test_valid_split_uses_train_stats(golden, shipped_data):
    _, arrs = golden
    tr, va, te = load_splits(shipped_data)
    assert torch.equal(va.get_full_batch()["macro_features"], gc.tensor(arrs["valid_macro_features"]))


def test_create_data_loaders_and_small_sample(golden, shipped_data):
    want, _ = golden
    args = []
    for s in ("train", "valid", "test"):
        args += list(_paths(shipped_data, s))
    B = create_data_loaders(*args)
    assert len(want["loaders_full_batch"]) == len(B)
    for da, db in zip(want["loaders_full_batch"], B):
        fb = db.get_full_batch()
        for k, v in da.items():
            assert v == gc.digest(fb[k]), k
    sa = want["small_sample_20_50"]
    sb = create_small_sample(B[0], 20, 50)
    for k in sa:
        assert sa[k] == gc.digest(sb[k]), k


def test_missing_sentinel_and_mask(tmp_path):
    T, N, F = 4, 5, 3
    data = np.random.RandomState(0).randn(T, N, F + 1).astype(np.float32)
    data[0, 1, 0] = -99.99                # missing return
    data[2, 3, 2] = -99.99                # one missing characteristic
    data[3, 4, 1] = np.nan
    np.savez(tmp_path / "c.npz", data=data, date=np.arange(T), variable=np.array(["RET", "a", "b", "c"]))
    ds = AssetPricingDataset(str(tmp_path / "c.npz"))
    b = ds.get_full_batch()
    m = b["mask"].numpy()
    assert not m[0, 1] and not m[2, 3] and not m[3, 4] and m.sum() == T * N - 3
    assert float(b["returns"][0, 1]) == 0.0 and torch.all(b["individual_features"][2, 3] == 0)
    assert "macro_features" not in b


def test_bf16_rounding_is_rne():
    x = np.array([1.0, 1.00390625, 1.01171875, -2.5, 3.140625, 1e-3, 0.0], np.float32)
    y = bf16_bits_to_f32(f32_to_bf16_bits(x))
    np.testing.assert_array_equal(y, torch.from_numpy(x).to(torch.bfloat16).float().numpy())


def test_prepare_split_compaction():
    rng = np.random.RandomState(1)
    T, N, F = 6, 9, 5
    feats = rng.randn(T, N, F).astype(np.float32)
    ret = rng.randn(T, N).astype(np.float32)
    mask = rng.rand(T, N) > 0.4
    mask[2] = False
    ps = prepare_split({"individual_features": feats, "returns": ret, "mask": mask,
                        "macro_features": rng.randn(T, 3).astype(np.float32)}, KP=64)
    assert ps.R == mask.sum() and ps.X.shape == (ps.R, 64)
    assert np.all(np.diff(ps.row_ptr) == mask.sum(1))
    tt, ii = ps.rowti[:, 0], ps.rowti[:, 1]
    assert np.all(mask[tt, ii])
    np.testing.assert_array_equal(bf16_bits_to_f32(ps.X[:, :F]), bf16_bits_to_f32(f32_to_bf16_bits(feats[tt, ii])))
    assert np.all(ps.X[:, F:] == 0)
    np.testing.assert_array_equal(ps.Rm.reshape(T, N), np.where(mask, ret, 0))


def test_uncompressed_npz_is_memory_mapped_and_equal(golden, shipped_data, tmp_path, monkeypatch):
    """An ``np.savez`` (stored) panel is mapped out of the archive, not read into RAM, and loads
    to the same tensors as the reference loader on the compressed original; the chunked masking
    pass gives the same result for any chunk size."""
    import deeplearninginassetpricing_paperreplication_amd.data.dataset as ds
    c, m = _paths(shipped_data, "train")
    arrs = gc.nan_panel_arrays(c)                          # a NaN return must be masked too
    plain = tmp_path / "Char_train.npz"
    np.savez(plain, **arrs)
    comp = tmp_path / "Char_train_c.npz"
    np.savez_compressed(comp, **arrs)
    assert isinstance(ds._npz_member(str(plain), "data"), np.memmap)
    assert not isinstance(ds._npz_member(str(comp), "data"), np.memmap)
    want = golden[0]["nan_panel_full_batch"]
    monkeypatch.setattr(ds, "_CHUNK_BYTES", 7 * 500 * 47 * 4)     # several uneven chunks
    for path in (plain, comp):
        got = AssetPricingDataset(str(path), m).get_full_batch()
        assert set(want) <= set(got)
        for k in want:
            assert want[k] == gc.digest(got[k]), (path.name, k)
