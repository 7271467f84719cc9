"""Host statement of the policy network's canonical float32 form (include/scanlib.h), in NumPy:

    x_k   = (r <= clip) ? r / scale : 1.0f,  r = scan[in_start + k]
    acc_j = +0.0f;  acc_j = fmaf(x_k, W[k][j], acc_j) for k = 0, 1, ..., K-1 in ascending order
    y_j   = acc_j + b_j;  ReLU: y_j > 0 ? y_j : 0.0f;  steer = y_0 of the last layer

Vectorised over cars and neurons, one k at a time.  ``fmaf`` is exact through round-to-odd: the f64 product of two
f32 values is exact, the f64 sum with the f32 addend is made odd-rounded from its TwoSum error, and the cast to f32
then rounds once, correctly (Boldo & Melquiond, "Emulation of FMA and correctly rounded sums: proved algorithms
using rounding to odd", IEEE TC 2008)."""
import numpy as np


def fmaf(a, b, c):
    """Correctly rounded float32 fma(a, b, c) of float32 arrays (broadcasting)."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b                                  # exact: 24 + 24 bits
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)              # TwoSum: s + e == p + c exactly (finite s)
        bits = s.view(np.uint64)
        fix = (e != 0) & ((bits & 1) == 0) & np.isfinite(s)
        if fix.any():
            # round to odd: step one ulp towards the error (|s| grows when e has s's sign)
            toward = np.where(np.signbit(e) == np.signbit(s), 1, -1).astype(np.int64)
            bits = np.where(fix, (bits.view(np.int64) + toward).view(np.uint64), bits)
            s = bits.view(np.float64)
    return s.astype(np.float32)


def policy_input(scans, in_start, K, clip=15.0, scale=15.0):
    """(n, size) float32 scans -> (n, K) float32 network inputs."""
    r = np.asarray(scans, np.float32)[:, in_start:in_start + K]
    with np.errstate(invalid="ignore"):
        keep = r <= np.float32(clip)
        # a correctly rounded f32 division: the f64 quotient of two f32 values rounded to f32 is the f32 quotient
        q = (r.astype(np.float64) / np.float64(np.float32(scale))).astype(np.float32)
    return np.where(keep, q, np.float32(1.0)).astype(np.float32)


def layer(x, W, b, relu):
    """One dense layer in the canonical form: (n, K) float32 -> (n, N) float32."""
    x = np.asarray(x, np.float32)
    W = np.asarray(W, np.float32)
    acc = np.zeros((x.shape[0], W.shape[1]), np.float32)
    for k in range(W.shape[0]):
        acc = fmaf(x[:, k:k + 1], W[k][None, :], acc)
    y = (acc + np.asarray(b, np.float32)[None, :]).astype(np.float32)
    if relu:
        y = np.where(y > 0, y, np.float32(0.0)).astype(np.float32)
    return y


def forward(scans, layers, relu, in_start=180, clip=15.0, scale=15.0):
    """Steers float32 (n,) of (n, size) scans."""
    x = policy_input(scans, in_start, layers[0][0].shape[0], clip, scale)
    for (W, b), r in zip(layers, relu):
        x = layer(x, W, b, r)
    return x[:, 0].copy()


def forward_f64(scans, layers, relu, in_start=180, clip=15.0):
    """The float64 forward pass of the same network (TF's answer up to its summation order): policy.py's input
    ``x if x <= 15.0 else 15.0`` divided by 15.0 in f64, then f64 matrix products."""
    r = np.asarray(scans, np.float32)[:, in_start:in_start + layers[0][0].shape[0]].astype(np.float64)
    with np.errstate(invalid="ignore"):
        x = np.where(r <= clip, r, clip) / clip
    for (W, b), rl in zip(layers, relu):
        x = x @ np.asarray(W, np.float64) + np.asarray(b, np.float64)
        if rl:
            x = np.maximum(x, 0.0)
    return x[:, 0].copy()


def load_fixture(path):
    """tests/golden/policy_mlp720.npz -> (layers [(W, b)], relu tuple)."""
    z = np.load(path)
    n = int(z["n_layers"])
    layers = [(z["W%d" % i], z["b%d" % i]) for i in range(n)]
    return layers, tuple(bool(v) for v in z["relu"])
