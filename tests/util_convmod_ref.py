"""numpy float64 restatement of the Conformer convolution module's inner half in training mode and of its backward
(include/daspeech_decode.h: dsp_dwconv_bn_silu_train_fwd / _bwd), on the channels-last layout:

    z[b,t,c] = sum_k w[c,k] * x[b, t+k-P, c]  (P = (K-1)/2, zero outside 0..T-1);  mean / biased var over the N = B*T values of a channel;
    zh = (z - mean) / sqrt(var + eps);  u = gamma*zh + beta;  y = u*sigmoid(u);  running buffers as nn.BatchNorm1d updates them.

tests/test_convmod_ref.py pins it to torch's float64 autograd on the CPU; the GPU tests measure the HIP operator against it."""
import numpy as np


def inputs(seed, B, T, C, K, mean_shift=0.5):
    """x [B,T,C], w [C,K], gamma, beta [C], grad_y [B,T,C], running_mean, running_var [C] — float64, of the sizes a trained layer shows"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, C)) + mean_shift * rng.standard_normal((1, 1, C))
    w = rng.standard_normal((C, K)) / np.sqrt(K)
    gamma = 1.0 + 0.3 * rng.standard_normal(C)
    beta = 0.3 * rng.standard_normal(C)
    gy = rng.standard_normal((B, T, C))
    rm = 0.2 * rng.standard_normal(C)
    rv = 1.0 + 0.5 * rng.random(C)
    return x, w, gamma, beta, gy, rm, rv


def depthwise(x, w):
    """z [B,T,C] float64"""
    B, T, C = x.shape
    K = w.shape[1]
    P = (K - 1) // 2
    xp = np.zeros((B, T + 2 * P, C))
    xp[:, P:P + T] = x
    z = np.zeros((B, T, C))
    for k in range(K):
        z += w[None, None, :, k] * xp[:, k:k + T]
    return z


def forward(x, w, gamma, beta, eps, running_mean=None, running_var=None, momentum=0.1):
    """-> dict(y, mean, invstd, var, running_mean, running_var) (the running entries None when not tracked)"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    B, T, C = x.shape
    N = B * T
    z = depthwise(x, w)
    mean = z.mean(axis=(0, 1))
    var = ((z - mean) ** 2).mean(axis=(0, 1))
    invstd = 1.0 / np.sqrt(var + eps)
    zh = (z - mean) * invstd
    u = gamma * zh + beta
    y = u / (1.0 + np.exp(-u))
    out = dict(y=y, mean=mean, invstd=invstd, var=var, zh=zh, u=u, running_mean=None, running_var=None)
    if running_mean is not None:
        out["running_mean"] = (1 - momentum) * np.asarray(running_mean, np.float64) + momentum * mean
        out["running_var"] = (1 - momentum) * np.asarray(running_var, np.float64) + momentum * var * N / (N - 1)
    return out


def backward(x, w, gamma, beta, eps, gy):
    """-> dict(dx [B,T,C], dw [C,K], dgamma [C], dbeta [C])"""
    x, w, gy = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(gy, np.float64)
    gamma = np.asarray(gamma, np.float64)
    B, T, C = x.shape
    K = w.shape[1]
    P = (K - 1) // 2
    N = B * T
    f = forward(x, w, gamma, beta, eps)
    zh, u, invstd = f["zh"], f["u"], f["invstd"]
    s = 1.0 / (1.0 + np.exp(-u))
    du = gy * s * (1 + u * (1 - s))
    dbeta = du.sum(axis=(0, 1))
    dgamma = (du * zh).sum(axis=(0, 1))
    dz = gamma * invstd * (du - dbeta / N - zh * dgamma / N)
    dzp = np.zeros((B, T + 2 * P, C))
    dzp[:, P:P + T] = dz
    xp = np.zeros((B, T + 2 * P, C))
    xp[:, P:P + T] = x
    dx = np.zeros((B, T, C))
    dw = np.zeros((C, K))
    for k in range(K):
        dx += w[None, None, :, k] * dzp[:, 2 * P - k:2 * P - k + T]          # dz[b, t-k+P]
        dw[:, k] = (dz * xp[:, k:k + T]).sum(axis=(0, 1))                     # x[b, t+k-P]
    return dict(dx=dx, dw=dw, dgamma=dgamma, dbeta=dbeta)


TIME_TILE = 8            # DSP_CONVMOD_TIME_TILE
CHUNK_TILES = 16         # DSP_CONVMOD_CHUNK_TILES

# (B, T, C, K): the edge shapes of the operator — every tap but one outside, T < P, T just past P, for every K one below / at / one above
# a multiple of the time tile, the minimum C, C not a multiple of 64 lanes, B = 1
EDGE_SHAPES = ([(2, 1, 8, 31), (3, 5, 8, 31), (2, 17, 16, 31)]
               + [(2, T, 8, K) for K in (3, 7, 15, 31) for T in (2 * TIME_TILE - 1, 2 * TIME_TILE, 2 * TIME_TILE + 1)]
               + [(2, 19, 264, 31), (2, 19, 256, 7), (1, 33, 8, 15)])
