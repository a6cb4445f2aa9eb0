"""numpy float64 restatements of the gradients of the variance-adaptor glue (csrc/tts_glue_grad.hip) and the error bound their GPU tests use.
tests/test_glue_grad_ref.py pins both to torch CPU float64 autograd, tests/test_gpu_glue_autograd.py compares the kernels with them."""
import numpy as np

# significand bits (hidden bit included) of the dtypes the kernels serve
SIGNIFICAND_BITS = {"float32": 24, "float16": 11, "bfloat16": 8}


def embed_grad_ref(grad_out, idx, rows):
    """gradient of `emb` in out[r] = x[r] + emb[idx[r]]: grad_emb[k] = sum of grad_out[r] over the rows r with idx[r] == k, in float64.
    grad_out [n,C], idx [n] -> [rows,C]; a bucket without a row stays zero"""
    g = np.asarray(grad_out, np.float64)
    out = np.zeros((rows, g.shape[1]), np.float64)
    for r, k in enumerate(np.asarray(idx).tolist()):
        out[k] += g[r]
    return out


def length_regulator_bwd_ref(grad_out, durations):
    """gradient of x in the length regulator (fastspeech2.py:98-114; phoneme t of sample b is repeated durations[b,t] times, frames after the
    sample's last one are padding): grad_x[b,t] = sum of the frames grad_out[b,f] that were copied from x[b,t], in float64.
    grad_out [B,maxlen,C], durations [B,N] -> [B,N,C].  Plain loops; padding frames are never read."""
    dur = np.asarray(durations)
    B, N = dur.shape
    C = grad_out.shape[2]
    out = np.zeros((B, N, C), np.float64)
    for b in range(B):
        f = 0
        for t in range(N):
            for _ in range(int(dur[b, t])):
                out[b, t] += np.asarray(grad_out[b, f], np.float64)
                f += 1
    return out


def sum_bound(m, abs_sum, ref, p):
    """bound on |got - ref| for a sum of m terms accumulated in fp32 in ANY order and rounded once to a dtype of p significand bits:
    every partial sum is at most sum|g_i| and each of the (at most m) fp32 additions rounds by at most 2^-24 of it; the final rounding adds
    2^-p of the result.   m * 2^-24 * sum|g_i| + 2^-p * |ref|     (m, abs_sum, ref broadcast elementwise)"""
    return np.asarray(m, np.float64) * 2.0 ** -24 * np.asarray(abs_sum, np.float64) + 2.0 ** -p * np.abs(np.asarray(ref, np.float64))


def embed_grad_terms(grad_out, idx, rows):
    """-> (m [rows,1] rows per bucket, abs_sum [rows,C] = sum of |grad_out| per bucket) for sum_bound"""
    m = np.bincount(np.asarray(idx), minlength=rows).astype(np.float64)[:, None]
    return m, embed_grad_ref(np.abs(np.asarray(grad_out, np.float64)), idx, rows)


def length_regulator_bwd_terms(grad_out, durations):
    """-> (m [B,N,1] frames per phoneme, abs_sum [B,N,C]) for sum_bound; padding frames (which may be NaN) are not read"""
    g = np.asarray(grad_out, np.float64)
    dur = np.asarray(durations)
    B, N = dur.shape
    a = np.zeros_like(g)
    for b in range(B):
        L = int(dur[b].sum())
        a[b, :L] = np.abs(g[b, :L])
    return dur.astype(np.float64)[:, :, None], length_regulator_bwd_ref(a, dur)
