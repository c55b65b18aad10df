"""Numpy float64 model of the MoE router entries (gq_moe_route, gq_moe_topk; include/gguf_mmq.h):
the logits, the selection keys, the stable top-k (descending key, ascending index on ties, NaN
last), the values and the weights, for both gating functions.  The GPU tests judge by it
(tests/test_gpu_moe_route.py); tests/test_moe_route_host.py checks it against hand-worked cases."""
import functools

import numpy as np

from utils.synth import random_activations

SOFTMAX, SIGMOID = 0, 1

# (E, H, S, N, seed): the shapes of the GPU tests
SHAPES = [(4, 64, 2, 3, 0),
          (3, 32, 3, 1, 0),       # S == E
          (8, 4096, 2, 1, 0),
          (8, 4096, 2, 4, 0),
          (60, 2048, 4, 8, 0),
          (128, 2048, 8, 5, 0),
          (160, 5120, 6, 2, 0),
          (256, 7168, 8, 4, 0),
          (8, 4096, 2, 64, 0),    # the last N on the device product
          (64, 2048, 6, 33, 3),
          (1024, 256, 64, 1, 160)]  # E and S at both limits
MIN_GAP = 1e-3       # between neighbours among the top S + 1 float64 logits of every shape above
MIN_KEY_GAP = 1e-4   # the same for sigmoid + bias keys
# the bias seed: the first 400 searched on the CPU for the largest key gap over all the shapes --
# 2.2e-4 with 235 (seed 1 leaves 6.3e-6 at the 1024-expert shape)
BIAS_SEED = 235


@functools.lru_cache(maxsize=None)
def inputs(E, H, N, seed):
    """(Wr fp32 (E, H), x fp16 (N, H)) of a case, read-only."""
    Wr = (np.random.default_rng(seed).standard_normal((E, H)) / np.sqrt(H)).astype(np.float32)
    x = random_activations(N, H, seed=seed)
    Wr.setflags(write=False)
    x.setflags(write=False)
    return Wr, x


def selection_bias(E, seed=BIAS_SEED):
    return np.random.default_rng(seed).uniform(-0.2, 0.2, E).astype(np.float32)


def logits(Wr, x):
    """x @ Wr^T in float64 (Wr as the entry reads it: pass the fp16-rounded matrix for an fp16 Wr)."""
    return x.astype(np.float64) @ Wr.astype(np.float64).T


def sigmoid(L):
    return 1.0 / (1.0 + np.exp(-np.asarray(L, np.float64)))


def keys(L, func, bias=None):
    """The selection keys in float64: the logits; sigmoid + bias when a bias is given."""
    L = np.asarray(L, np.float64)
    if bias is None:
        return L
    assert func == SIGMOID
    return sigmoid(L) + np.asarray(bias, np.float64)[None, :]


def topk(K, S):
    """Per row the S indices of largest key: descending key, ascending index among equal keys,
    NaN keys after every number (ascending index among themselves)."""
    K = np.asarray(K, np.float64)
    out = np.empty((K.shape[0], S), np.int32)
    for n, row in enumerate(K):
        nan = np.isnan(row)
        neg = np.where(nan, 0.0, -row)
        order = np.lexsort((np.arange(row.size), neg, nan))  # last key first: NaN flag, then -key, then index
        out[n] = order[:S]
    return out


def values(L, func):
    """softmax over all experts with the row maximum subtracted, or sigmoid."""
    L = np.asarray(L, np.float64)
    if func == SIGMOID:
        return sigmoid(L)
    p = np.exp(L - L.max(axis=1, keepdims=True))
    return p / p.sum(axis=1, keepdims=True)


def weights(L, ids, func, norm, scale):
    v = np.take_along_axis(values(L, func), ids.astype(np.int64), axis=1)
    if norm:
        v = v / v.sum(axis=1, keepdims=True)
    return v * scale


def route(L, S, func=SOFTMAX, norm=True, scale=1.0, bias=None):
    """(ids, weights) of gq_moe_topk on the logits L."""
    ids = topk(keys(L, func, bias), S)
    return ids, weights(L, ids, func, norm, scale)


def top_gap(K, S):
    """The smallest difference between neighbours among each row's S + 1 largest keys."""
    K = np.asarray(K, np.float64)
    top = -np.sort(-K, axis=1)[:, :min(S + 1, K.shape[1])]
    return float(np.min(top[:, :-1] - top[:, 1:])) if top.shape[1] > 1 else float("inf")


def ulp16(a, b):
    """Distance in fp16 steps between two fp16 arrays (finite values)."""
    def lin(v):
        u = np.asarray(v, np.float16).view(np.uint16).astype(np.int32)
        return np.where(u & 0x8000, -(u & 0x7fff), u)
    return np.abs(lin(a) - lin(b))
