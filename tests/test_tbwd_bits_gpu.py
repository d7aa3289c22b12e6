"""Bit-level pin of the one-pass SDF tower backward (``csrc/k_tbwd.hip``) on a real MI355X.

Instruction-level work on the kernel must not change any fp32 summation order (per-wave tile order,
the four-wave tree, the R-only slab partition, the output-row and bias sums), so the SDF-scope
gradients after ``backward_only`` -- the tower's weights and biases and, through dL/d(per-period
inputs), the macro LSTM's -- keep the bits recorded in ``tests/golden/tbwd_parent_digests.json``.

The default fine-slab count gives every wave 0 or 1 tile at this panel size, so every
architecture also runs with 1, 2 and 8 coarse slabs (waves of 30-31, 15-16 and 3-4 tiles, always
waves of both lengths): both prefetch slots, their rotation and the drain are exercised. The intended tile counts are asserted from R and the engine's launch
shape, so a later change of the partition cannot hollow the cases out.

Regenerating the digests (only when a summation order is changed on purpose), on an MI355X:
    python tests/test_tbwd_bits_gpu.py
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from deeplearninginassetpricing_paperreplication_amd.config import default_cli_config  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.data.synthetic import generate_panel_fast  # noqa: E402
from deeplearninginassetpricing_paperreplication_amd.models.gan import AssetPricingGAN  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "tbwd_parent_digests.json")

ARCHS = {
    "h64x2": ([64, 64], [4]),
    "h64x1": ([64], [4]),
    "h64x3": ([64] * 3, [4]),
    "h64x4": ([64] * 4, [4]),
    "h48_32": ([48, 32], [2, 2]),
}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeplearninginassetpricing_paperreplication_amd.ops import native
    native.load(required=True)


_PANELS = {}


def _panel(name):
    """base: the panel of tests/test_tbwd_gpu.py::_batch; ragged: 677 stocks (the row count is no
    multiple of 32); empty: the base panel with period 5 fully masked."""
    if name not in _PANELS:
        N = 677 if name == "ragged" else 700
        ret, feats, mask, mac = generate_panel_fast(48, N, 46, 8, seed=0)
        mac = (mac - mac.mean(0)) / (mac.std(0, unbiased=False) + 1e-8)
        if name == "empty":
            mask = mask.clone()
            mask[5] = False
        _PANELS[name] = {"returns": ret, "individual_features": feats, "mask": mask, "macro_features": mac}
    return _PANELS[name]


def _cases():
    c = []
    # every architecture, both phases, without and with dropout, the default partition
    for arch in ARCHS:
        for phase in (1, 3):
            for dropout in (0.0, 0.05):
                c.append((arch, phase, dropout, 1, "base", 0, 0))
    # several tiles per wave: 1, 2 and 8 coarse slabs, every architecture, the ragged panel
    for arch in ARCHS:
        for coarse in (1, 2, 8):
            c.append((arch, 3, 0.05, 1, "ragged", coarse, 0))
    # an empty period, with one and with many tiles per wave
    c.append(("h64x2", 3, 0.05, 1, "empty", 0, 0))
    c.append(("h64x2", 1, 0.0, 1, "empty", 2, 0))
    # three models in one launch
    c.append(("h64x2", 3, 0.05, 3, "base", 0, 0))
    c.append(("h64x2", 1, 0.05, 3, "ragged", 2, 0))
    c.append(("h64x3", 3, 0.0, 3, "base", 8, 0))
    # wide layer-0 path (ZIN)
    for phase in (1, 3):
        c.append(("h64x2", phase, 0.05, 1, "base", 0, 1))
    c.append(("h64x2", 3, 0.05, 1, "ragged", 2, 1))
    return c


CASES = _cases()


def _case_id(case):
    arch, phase, dropout, G, panel, coarse, wide = case
    return f"{arch}-p{phase}-d{dropout:g}-G{G}-{panel}-c{coarse}-w{wide}"


def _setenv(monkeypatch, key, val):
    if monkeypatch is None:
        os.environ[key] = val
    else:
        monkeypatch.setenv(key, val)


def _delenv(monkeypatch, key):
    if monkeypatch is None:
        os.environ.pop(key, None)
    else:
        monkeypatch.delenv(key, raising=False)


def _digests(case, monkeypatch=None):
    from deeplearninginassetpricing_paperreplication_amd.engine.runner import GANEngine
    arch, phase, dropout, G, panel, coarse, wide = case
    hidden, rnn = ARCHS[arch]
    _setenv(monkeypatch, "DLAP_TBWD", "1")
    for key, val in (("DLAP_NSLAB_COARSE", coarse), ("DLAP_WIDE", wide)):
        if val:
            _setenv(monkeypatch, key, str(val))
        else:
            _delenv(monkeypatch, key)
    cfg = default_cli_config(8, 46, hidden_dim=hidden, rnn_dim=rnn, dropout=dropout)
    b = _panel(panel)
    spec = AssetPricingGAN(cfg).spec
    eng = GANEngine(spec, G, max_epochs=8)
    assert int(eng.desc["tbwd"]) == 1 and int(eng.desc["wide"]) == wide
    eng.set_data(b, b, b)
    for g in range(G):
        torch.manual_seed(100 + g)
        eng.set_model(g, AssetPricingGAN(cfg), 11 + g)
    eng.eng.backward_only(phase)
    # the launch shape this case is meant to run at: nfine workgroups of 4 waves, wave w of workgroup
    # v takes tiles 4v + w + 4 nfine k
    R = int(b["mask"].sum())
    ntiles = (R + 31) // 32
    nfine = int(eng.eng.fused_info()["bwd_nfine"])
    want = 4 * max(1, min(coarse if coarse else 64, ((ntiles + 3) // 4 + 3) // 4))
    assert nfine == want, (nfine, want)
    waves = 4 * nfine
    most, least = -(-ntiles // waves), ntiles // waves
    if coarse == 0:
        assert most == 1                          # the default partition: 0 or 1 tile per wave
    else:
        # 30-31, 15-16 and 3-4 tiles per wave (480..499 tiles): waves of both lengths in every case
        assert least == {1: 30, 2: 15, 8: 3}[coarse] and most == least + 1, (least, most)
    if panel == "ragged":
        assert R % 32 != 0                        # a partial last tile
    P_sdf = spec.param_counts()[0]
    out = []
    for g in range(G):
        gr = np.ascontiguousarray(eng.eng.get_grads(g)[:P_sdf], dtype=np.float32)
        assert np.isfinite(gr).all() and np.abs(gr).max() > 0
        out.append(hashlib.sha256(gr.tobytes()).hexdigest())
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["digests"]


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_sdf_gradient_bits_equal_recorded(monkeypatch, golden, case):
    assert _digests(case, monkeypatch) == golden[_case_id(case)]


def test_every_case_has_a_golden(golden):
    assert sorted(golden) == sorted(_case_id(c) for c in CASES)


if __name__ == "__main__":
    rec = {"note": ["sha256 of Engine.get_grads(g)[:P_sdf] (float32 bytes) after backward_only(phase), one per model;",
                    "recorded on an MI355X from the commit before the tile-loop rework of csrc/k_tbwd.hip.",
                    "Regenerate with `python tests/test_tbwd_bits_gpu.py` only when a summation order changes on purpose."],
           "digests": {_case_id(c): _digests(c) for c in CASES}}
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec['digests'])} cases -> {out}")
