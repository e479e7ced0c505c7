"""The planar Q4_K / Q5_K scale field as four 24-bit records, on the device.

* canonical -> planar -> canonical gives the original bytes back (get_tensor reads weights back) for Q4_K, Q5_K and Q6_K, at K = 256,
  2048 and the Llama shapes;
* the planar rows the load-time pack writes are exactly the numpy restatement of the layout (tests/test_kquant_records.py);
* mi355q_mul_mat at N = 1, 2, 8 (GEMV tier) and 16, 64 (Q4_K: integer matrix cores, Q5_K: bf16 matrix cores) gives the same bits as the
  library gave before the scale field was rearranged (tests/golden/kquant_records_outputs.npz, written by
  tests/golden/make_kquant_records_golden.py with that library)."""
from pathlib import Path

import numpy as np
import pytest

import oracle
from kquant_cases import KS, NS, TYPES, M, case_inputs, golden_key
from qdata import random_blocks
from test_kquant_records import to_records

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "kquant_records_outputs.npz"


@pytest.fixture(scope="module")
def G():
    import torch
    import ggml_mi355 as g
    assert torch.cuda.is_available() and g.lib().mi355q_device_count() >= 1
    return g


@pytest.mark.parametrize("t", (oracle.Q4_K, oracle.Q5_K, oracle.Q6_K), ids=lambda t: oracle.TYPE_NAMES[t])
@pytest.mark.parametrize("k", (256, 2048, 4096, 14336))
def test_round_trip(G, t, k):
    rng = np.random.default_rng(k + t)
    w = random_blocks(t, 48, k, rng)
    q = G.QWeight.from_host(t, w, 48, k)
    assert np.array_equal(q.to_host(), w)


@pytest.mark.parametrize("t", (oracle.Q4_K, oracle.Q5_K), ids=lambda t: oracle.TYPE_NAMES[t])
@pytest.mark.parametrize("k", (256, 4096, 14336))
def test_planar_bytes(G, t, k):
    rng = np.random.default_rng(3 * k + t)
    rows = 16
    w = random_blocks(t, rows, k, rng)
    q = G.QWeight.from_host(t, w, rows, k)
    assert G.is_planar(t, k)
    dev = q.data[: q.nbytes].cpu().numpy().reshape(rows, -1)
    nb = k // 256
    blk = w.reshape(rows, nb, -1)
    hdr = blk[:, :, :16].copy()
    hdr[:, :, 4:16] = to_records(blk[:, :, 4:16].reshape(-1, 12)).reshape(rows, nb, 12)
    if t == oracle.Q4_K:      # [qs 128 nb][hdr 16 nb]
        want = np.concatenate([blk[:, :, 16:144].reshape(rows, -1), hdr.reshape(rows, -1)], axis=1)
    else:                     # [qs 128 nb][qh 32 nb][hdr 16 nb]
        want = np.concatenate([blk[:, :, 48:176].reshape(rows, -1), blk[:, :, 16:48].reshape(rows, -1), hdr.reshape(rows, -1)], axis=1)
    assert np.array_equal(dev, want)


@pytest.mark.parametrize("t", TYPES, ids=lambda t: oracle.TYPE_NAMES[t])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_mul_mat_bits_unchanged(G, t, k, n):
    import torch
    w, x = case_inputs(t, k, n)
    y = G.mul_mat(G.QWeight.from_host(t, w, M, k), torch.from_numpy(x).cuda()).cpu().numpy()
    want = np.load(GOLDEN)[golden_key(t, k, n)]
    assert y.shape == want.shape
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32))
