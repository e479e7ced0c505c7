"""The float-weight GEMV's references (mi355q_mul_mat_fw): numpy restatements of the CPU's bf16 arithmetic.  The f16 side is
oracle.glue.vec_dot_f16_simd as it is.  tests/test_fw_ref_cpu.py holds them to the recorded outputs of the reference CPU backend."""
import numpy as np

f32 = np.float32


def f32_to_bf16(x: np.ndarray) -> np.ndarray:
    """ggml_compute_fp32_to_bf16 (ggml-impl.h): round to nearest even on the bits, subnormals kept, a NaN made quiet as (bits >> 16) | 0x40."""
    u = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.uint64)
    rne = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where((u & 0x7FFFFFFF) > 0x7F800000, ((u >> 16) | 0x40).astype(np.uint16), rne)


def bf16_to_f32(b: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(b, np.uint16).astype(np.uint32) << 16).view(f32)


def vec_dot_bf16_avx2(w_bits: np.ndarray, x_bits: np.ndarray) -> np.ndarray:
    """ggml_vec_dot_bf16, AVX2 branch (ggml-cpu/vec.cpp): rows w_bits [R, n] against x_bits [n] (bf16 bits) -> [R] f32.  Element i of each 32-chunk goes
    to accumulator (i % 32) / 8, lane i % 8 by a multiply THEN an add (both rounded to f32), chunks in order; (c1 + c3) + (c2 + c4); high half + low
    half; movehl; movehdup; the tail past the last whole chunk is added in double, one f32-rounded product at a time."""
    w = bf16_to_f32(w_bits).astype(np.float64); x = bf16_to_f32(x_bits).astype(np.float64)
    R, n = w.shape
    npb = n & ~31
    acc = np.zeros((R, 4, 8), f32)
    with np.errstate(all="ignore"):
        for b0 in range(0, npb, 32):
            prod = (w[:, b0:b0 + 32] * x[b0:b0 + 32]).astype(f32).reshape(R, 4, 8)      # (exact in f64, rounded once to f32)
            acc = prod + acc
        c = (acc[:, 0] + acc[:, 2]) + (acc[:, 1] + acc[:, 3])                             # [R, 8]
        g = c[:, 4:] + c[:, :4]
        res = (g[:, 0] + g[:, 2]) + (g[:, 1] + g[:, 3])
        sumf = res.astype(np.float64)
        for i in range(npb, n):
            sumf = sumf + (w[:, i] * x[i]).astype(f32).astype(np.float64)
    return sumf.astype(f32)


def mul_mat_bf16(w_bits: np.ndarray, x: np.ndarray) -> np.ndarray:
    """[N, M] f32: every x row rounded by f32_to_bf16, then vec_dot_bf16_avx2 per weight row."""
    return np.stack([vec_dot_bf16_avx2(w_bits, f32_to_bf16(xr)) for xr in np.asarray(x, f32)])


def mul_mat_f16(w: np.ndarray, x: np.ndarray) -> np.ndarray:
    """[N, M] f32: every x row rounded to f16 (nearest even), then ggml_vec_dot_f16 (oracle.glue.vec_dot_f16_simd) per weight row."""
    from oracle import glue
    with np.errstate(all="ignore"):
        return np.stack([glue.vec_dot_f16_simd(np.asarray(w, np.float16), np.asarray(xr, f32).astype(np.float16)) for xr in np.asarray(x, f32)])


def same_bits(got: np.ndarray, want: np.ndarray) -> bool:
    """Bit equality of two f32 arrays.  Where the reference is a NaN the result must be a NaN: which NaN an addition or multiplication returns is
    not fixed by IEEE 754 (sign and payload differ between x86 and the GPU, and the f64 restatement gives neither), every other value is."""
    got = np.ascontiguousarray(got, f32); want = np.ascontiguousarray(want, f32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))
