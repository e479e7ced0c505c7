"""mi355q_mul_mat_fw_path: which calls the float-weight streaming GEMV takes, asked from numbers alone (no device, nothing dereferenced)."""
import pytest

import ggml_mi355 as G

W, X, Y = 0x7000_0000_0000, 0x7100_0000_0000, 0x7200_0000_0000              # only addresses
TYPES = [(1, "f16"), (30, "bf16")]


def path(t, m, n, k, w=W, ws=None, x=X, xs=None, y=Y, ys=None, flags=0):
    return G.mul_mat_fw_path(t, w, 2 * k if ws is None else ws, x, 4 * k if xs is None else xs, y, 4 * m if ys is None else ys, m, n, k, flags)


@pytest.mark.parametrize("t,name", TYPES)
@pytest.mark.parametrize("m,n,k", [(1, 1, 32), (4096, 1, 4096), (17, 8, 64)])
def test_stream(t, name, m, n, k):
    assert path(t, m, n, k) == G.FW_PATH_STREAM
    for fl in G.FW_ROWS_PER_WAVE:
        assert path(t, m, n, k, flags=fl) == G.FW_PATH_STREAM


@pytest.mark.parametrize("t,name", TYPES)
def test_unsupported(t, name):
    U = G.ERR_UNSUPPORTED
    m, n, k = 17, 2, 64
    assert path(t, m, n, 100) == U and path(t, m, n, 8) == U                 # K % 32 (the tail in double stays with op_mul_mat_f), K < 32
    assert path(t, m, 0, k) == U and path(t, m, 9, k) == U
    assert path(t, m, n, k, w=W + 8) == U                                    # bit 3 of the address
    assert path(t, m, n, k, ws=2 * k + 8) == U and path(t, m, n, k, ws=2 * k - 16) == U
    assert path(t, m, n, k, ws=2 * k + 16) == G.FW_PATH_STREAM
    assert path(t, m, n, k, xs=4 * k + 2) == U
    assert path(t, m, n, k, xs=4 * k + 4) == G.FW_PATH_STREAM
    assert path(t, m, n, k, ys=4 * m - 4) == U and path(t, m, n, k, ys=4 * m + 4) == G.FW_PATH_STREAM
    assert path(t, 0, n, k) == U
    assert path(t, m, n, k, flags=4) == U
    assert b"mul_mat_fw" in G.lib().mi355q_last_error()


def test_short_wide_batches_stay_with_the_old_kernel():
    """measured slower (profiles/fw_stream.md): 4 or more columns over a short, large matrix"""
    for t, _ in TYPES:
        assert path(t, 4096, 8, 4096) == G.ERR_UNSUPPORTED and path(t, 4096, 4, 14336) == G.ERR_UNSUPPORTED
        assert path(t, 4096, 3, 14336) == G.FW_PATH_STREAM and path(t, 14336, 8, 4096) == G.FW_PATH_STREAM and path(t, 1031, 8, 2080) == G.FW_PATH_STREAM


def test_other_types_are_refused():
    for t in (0, 8):
        assert path(t, 17, 2, 64) == G.ERR_UNSUPPORTED
    assert G.lib().mi355q_type_supported(1) == 0 and G.lib().mi355q_type_supported(30) == 0      # not types of the quantized path
    assert {"mi355q_mul_mat_fw", "mi355q_mul_mat_fw_path"} <= set(G.ABI_SYMBOLS)
