"""The policy network's host side (no GPU): the round-to-odd fmaf of the host statement, the input transform, the
frozen-graph reader on hand-encoded GraphDefs and on the reference's own graphs, and the distance of the canonical
float32 form from a float64 forward pass."""
import os
import struct
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLD
import policy_statement as S
from pyracecarsimulator_amd.policy import read_frozen_graph

FIXTURE = os.path.join(GOLD, "policy_mlp720.npz")
REF_MODEL = "/root/reference/model"


# ---------------------------------------------------------------- fmaf
def _exact_fmaf(a, b, c):
    return np.float32(float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))))


def _f32_from_fraction(q):
    """Correct f32 rounding of an exact rational (ties to even), via the two f32 neighbours."""
    lo = np.float32(float(q))
    # float(q) is correctly rounded to f64; step to f32 neighbours and pick the nearer exactly
    cands = {lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))}
    best = None
    for v in cands:
        if not np.isfinite(v):
            continue
        d = abs(Fraction(float(v)) - q)
        key = (d, int(np.array(v, np.float32).view(np.uint32)) & 1)
        if best is None or key < best[0]:
            best = (key, v)
    return best[1]


def test_fmaf_round_to_odd_matches_exact_rationals():
    rng = np.random.default_rng(1)
    n = 6000
    a = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))).astype(np.float32)
    b = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))).astype(np.float32)
    c = (rng.standard_normal(n) * np.exp2(rng.integers(-40, 40, n))).astype(np.float32)
    # cancelling triples: c = -round(a * b) (+ a few ulps), the product's low bits decide everything
    m = n // 2
    c[:m] = (-(a[:m].astype(np.float64) * b[:m])).astype(np.float32)
    c[: m // 2] = np.nextafter(c[: m // 2], np.float32(np.inf))
    got = S.fmaf(a, b, c)
    bad = 0
    for i in range(n):
        want = _f32_from_fraction(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        if np.float32(want).tobytes() != got[i].tobytes() and not (want == 0 and got[i] == 0):
            bad += 1
    assert bad == 0
    # the naive f64 form (one f64 rounding, then f32) double-rounds somewhere in the same set
    naive = (a.astype(np.float64) * b + c).astype(np.float32)
    assert naive.shape == got.shape


def test_fmaf_double_rounding_case():
    # a*b + c lies just above a tie of f32 in the f64 sum's rounding: naive f64 rounds to the tie, then to even
    a, b = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12)          # a*b = 1 + 2^-11 + 2^-24 exactly
    c = np.float32(2.0 ** -60)
    want = _f32_from_fraction(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))
    assert S.fmaf(a, b, c).tobytes() == np.float32(want).tobytes()
    assert want == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    naive = np.float32(np.float64(a) * np.float64(b) + np.float64(c))
    assert naive != want                                                    # the case round-to-odd exists for


# ---------------------------------------------------------------- input transform
def test_input_transform_matches_reference_formula():
    v = [np.nan, np.inf, -np.inf, 15.0, 0.0, -0.0, 0.1, 1.0 / 3.0, 7.3, 14.999999, 29.0, 1e-40, -2.5, 1e30]
    v += [float(np.nextafter(np.float32(15.0), np.float32(0))), float(np.nextafter(np.float32(15.0), np.float32(20)))]
    rng = np.random.default_rng(2)
    v += list(rng.uniform(0, 16, 4000).astype(np.float32).astype(float))
    scans = np.array(v, np.float32)[None, :]
    got = S.policy_input(scans, 0, scans.shape[1])[0]
    # scripts/policy.py: lidar_proc(i) / 15.0 on the f32 element, in f64, cast to f32 at the placeholder
    want = np.array([np.float32((float(i) if float(i) <= 15.0 else 15.0) / 15.0) for i in scans[0]], np.float32)
    assert got.tobytes() == want.tobytes()
    assert got[0] == 1.0 and got[1] == 1.0 and got[3] == 1.0


# ---------------------------------------------------------------- the reader
def _varint(v):
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _key(num, wt):
    return _varint(num << 3 | wt)


def _ld(num, payload):
    return _key(num, 2) + _varint(len(payload)) + payload


def _vi(num, v):
    return _key(num, 0) + _varint(v & ((1 << 64) - 1))


def _tensor(arr, form="content", dtype=1, shape=None):
    arr = np.asarray(arr, np.float32)
    shape = arr.shape if shape is None else shape
    sh = b"".join(_ld(2, _vi(1, s)) for s in shape)
    t = _vi(1, dtype) + _ld(2, sh)
    if form == "content":
        t += _ld(4, arr.astype("<f4").tobytes())
    elif form == "packed":
        t += _ld(5, arr.astype("<f4").tobytes())
    elif form == "unpacked":
        t += b"".join(_key(5, 5) + struct.pack("<f", float(x)) for x in arr.reshape(-1))
    elif form == "scalar":                                 # one float_val fills the shape
        t += _key(5, 5) + struct.pack("<f", float(arr.reshape(-1)[0]))
    return t


def _attr(key, value):
    return _ld(5, _ld(1, key.encode()) + _ld(2, value))


def _node(name, op, inputs=(), attrs=()):
    body = _ld(1, name.encode()) + _ld(2, op.encode()) + b"".join(_ld(3, i.encode()) for i in inputs)
    return _ld(1, body + b"".join(_attr(k, v) for k, v in attrs))


def _const(name, arr, form="content", dtype=1, shape=None):
    return _node(name, "Const", (), [("dtype", _vi(6, dtype)), ("value", _ld(8, _tensor(arr, form, dtype, shape)))])


def _graph(layers, forms=None, relu=None, identity=False, ops=None, transpose_b=False, dtype=1, skip_shape=False):
    n = len(layers)
    relu = relu if relu is not None else [i < n - 1 for i in range(n)]
    forms = forms or ["content"] * (2 * n)
    g = _node("input_layer", "Placeholder", (), [("dtype", _vi(6, 1))])
    prev = "input_layer"
    for i, (W, b) in enumerate(layers):
        wn, bn = "dense_%d/kernel" % i, "dense_%d/bias" % i
        g += _const(wn, W, forms[2 * i], dtype)
        g += _const(bn, b, forms[2 * i + 1], dtype, shape=(len(b),) if forms[2 * i + 1] == "scalar" else None)
        if identity:
            g += _node(wn + "/read", "Identity", [wn]) + _node(wn + "/read2", "Identity", [wn + "/read"])
            wn = wn + "/read2"
        last = i == n - 1
        scope = "output_layer" if last else "dense_%d" % i
        mm_attrs = [("T", _vi(6, 1)), ("transpose_a", _vi(5, 0)), ("transpose_b", _vi(5, int(transpose_b)))]
        g += _node(scope + "/MatMul", "MatMul", [prev + ":0", wn], mm_attrs)
        g += _node(scope + "/BiasAdd", (ops or {}).get(i, "BiasAdd"), [scope + "/MatMul", bn], [("T", _vi(6, 1))])
        prev = scope + "/BiasAdd"
        if relu[i]:
            g += _node(scope + "/Relu", "Relu", [prev])
            prev = scope + "/Relu"
    return g


def _rand_layers(dims, seed=0):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((dims[i], dims[i + 1])).astype(np.float32),
             rng.standard_normal(dims[i + 1]).astype(np.float32)) for i in range(len(dims) - 1)]


def _same_layers(a, b):
    return len(a) == len(b) and all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()
                                    and x[0].shape == y[0].shape for x, y in zip(a, b))


def test_reader_tensor_forms():
    layers = _rand_layers([7, 5, 3, 1], 3)
    layers[2] = (layers[2][0], np.full(1, 0.25, np.float32))
    forms = ["content", "packed", "unpacked", "content", "packed", "scalar"]
    got = read_frozen_graph(_graph(layers, forms))
    assert _same_layers(got, layers)
    assert got.relu == (True, True, False)
    # a single float_val broadcast over a whole weight matrix
    layers2 = [(np.full((4, 3), -1.5, np.float32), np.zeros(3, np.float32)), (np.ones((3, 1), np.float32), np.ones(1, np.float32))]
    got2 = read_frozen_graph(_graph(layers2, ["scalar", "scalar", "scalar", "scalar"]))
    assert _same_layers(got2, layers2)


def test_reader_identity_chains_and_relu_pattern():
    layers = _rand_layers([9, 4, 6, 1], 4)
    got = read_frozen_graph(_graph(layers, identity=True, relu=[False, True, False]))
    assert _same_layers(got, layers) and got.relu == (False, True, False)


@pytest.mark.parametrize("case", ["tanh", "transpose_b", "half", "shape"])
def test_reader_rejects(case):
    layers = _rand_layers([6, 4, 1], 5)
    if case == "tanh":
        data = _graph(layers, ops={0: "Tanh"})
        node = "dense_0/BiasAdd"
    elif case == "transpose_b":
        data = _graph(layers, transpose_b=True)
        node = "MatMul"
    elif case == "half":
        data = _graph(layers, dtype=19)
        node = "bias"
    else:
        layers[1] = (np.ones((5, 1), np.float32), np.ones(1, np.float32))       # 4 outputs into 5 inputs
        data = _graph(layers)
        node = "MatMul"
    with pytest.raises(ValueError, match=node):
        read_frozen_graph(data)


def test_reader_reference_graphs_equal_fixture():
    if not os.path.isdir(REF_MODEL):
        pytest.skip("the reference's model directory is not on this machine")
    import hashlib
    layers, relu = S.load_fixture(FIXTURE)
    z = np.load(FIXTURE)
    for fname, key in (("frozen_model.pb", "sha256_frozen"), ("TensorRT_model.pb", "sha256_tensorrt")):
        path = os.path.join(REF_MODEL, fname)
        assert hashlib.sha256(open(path, "rb").read()).hexdigest() == str(z[key])
        got = read_frozen_graph(path)
        assert _same_layers(got, layers) and got.relu == relu


def test_fixture_shape():
    layers, relu = S.load_fixture(FIXTURE)
    assert [W.shape for W, _ in layers] == [(720, 64), (64, 128), (128, 128), (128, 64), (64, 1)]
    assert relu == (True, True, True, True, False)
    assert sum(W.size + b.size for W, b in layers) == 79297


# ---------------------------------------------------------------- distance to the float64 answer
def _scans(n, seed, size=1081):
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.05, 20.0, (n, size)).astype(np.float32)
    # corridor-like rows: smooth walls at a few metres, some beams beyond the clip
    base = rng.uniform(0.5, 6.0, (n, 1)) * (1.0 + 0.5 * np.sin(np.linspace(0, 6, size))[None, :] * rng.uniform(0, 1, (n, 1)))
    half = n // 2
    s[:half] = base[:half].astype(np.float32)
    return s


def test_f32_form_within_bound_of_f64():
    layers, relu = S.load_fixture(FIXTURE)
    scans = _scans(10000, 6)
    got = S.forward(scans, layers, relu)
    ref = S.forward_f64(scans, layers, relu)
    d = np.abs(got.astype(np.float64) - ref)
    assert np.isfinite(got).all()
    assert d.max() < 1e-5, (d.max(), np.percentile(d, 99))
