"""The steering policy network on the GPU — drop-in for the reference's ``scripts/policy.py``.

The reference loads a frozen TF-1 graph (``model/frozen_model.pb``, or the same weights in
``model/TensorRT_model.pb``) and runs it on ONE scan per call: ``Policy().predict_action(lidar)``
feeds ``lidar[180:900]``, clipped at 15 m and divided by 15, to a 720 -> 64 -> 128 -> 128 -> 64 -> 1
ReLU MLP and returns one steering angle (scripts/policy.py:17-33; driven at scripts/policy_driver.py:30-49,
used by MCTS at scripts/mcts.py:252-256).  Here the graph is read without TF (``read_frozen_graph``: the
protobuf wire format by hand), and the network runs in one HIP launch for any number of scans
(``csrc/policy_kernels.h``), host or device resident.  Results follow the project's canonical float32 form
(include/scanlib.h): a k-ordered ``fmaf`` chain per neuron, bit-identical on every path.
"""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np

from . import _lib

#: the reference's tensor names (scripts/policy.py:25-26)
INPUT_NAME = "input_layer"
OUTPUT_NAME = "output_layer/BiasAdd"

DT_FLOAT = 1


# ---------------------------------------------------------------- protobuf wire format
def _varint(buf, i):
    shift = val = 0
    while True:
        if i >= len(buf):
            raise ValueError("truncated varint")
        b = buf[i]
        i += 1
        val |= (b & 0x7F) << shift
        if not b & 0x80:
            return val, i
        shift += 7


def _fields(buf):
    """(field number, wire type, value) of one message: ints for varint / fixed, bytes for length-delimited."""
    i, n = 0, len(buf)
    while i < n:
        key, i = _varint(buf, i)
        num, wt = key >> 3, key & 7
        if wt == 0:
            val, i = _varint(buf, i)
        elif wt == 1:
            val, i = buf[i:i + 8], i + 8
        elif wt == 2:
            ln, i = _varint(buf, i)
            val, i = buf[i:i + ln], i + ln
        elif wt == 5:
            val, i = buf[i:i + 4], i + 4
        else:
            raise ValueError("unsupported protobuf wire type %d" % wt)
        if i > n:
            raise ValueError("truncated protobuf field %d" % num)
        yield num, wt, val


def _tensor(buf, where):
    """TensorProto -> float32 ndarray (dtype=1, tensor_shape=2, tensor_content=4, float_val=5)."""
    dtype, shape, content, vals = 0, [], None, []
    for num, wt, val in _fields(buf):
        if num == 1 and wt == 0:
            dtype = val
        elif num == 2 and wt == 2:
            for dn, dw, dv in _fields(val):
                if dn == 2 and dw == 2:
                    size = 0
                    for sn, sw, sv in _fields(dv):
                        if sn == 1 and sw == 0:
                            size = sv - (1 << 64) if sv >= 1 << 63 else sv
                    shape.append(size)
        elif num == 4 and wt == 2:
            content = bytes(val)
        elif num == 5 and wt == 2:              # packed
            vals.extend(struct.unpack("<%df" % (len(val) // 4), val))
        elif num == 5 and wt == 5:              # unpacked
            vals.append(struct.unpack("<f", val)[0])
    if dtype != DT_FLOAT:
        raise ValueError("node %r: tensor dtype %d is not DT_FLOAT" % (where, dtype))
    if any(s < 0 for s in shape):
        raise ValueError("node %r: tensor shape %s is not fully defined" % (where, shape))
    count = int(np.prod(shape)) if shape else 1
    if content is not None:
        a = np.frombuffer(content, dtype="<f4").astype(np.float32)
    elif len(vals) == 1:
        a = np.full(count, vals[0], dtype=np.float32)    # one value fills the shape, as TF does
    else:
        a = np.array(vals, dtype=np.float32)
    if a.size != count:
        raise ValueError("node %r: %d values for shape %s" % (where, a.size, shape))
    return a.reshape(shape)


class _Node:
    __slots__ = ("name", "op", "inputs", "attr")

    def __init__(self, buf):
        self.name, self.op, self.inputs, self.attr = "", "", [], {}
        for num, wt, val in _fields(buf):
            if wt != 2:
                continue
            if num == 1:
                self.name = bytes(val).decode()
            elif num == 2:
                self.op = bytes(val).decode()
            elif num == 3:
                s = bytes(val).decode()
                if not s.startswith("^"):                 # (control dependencies carry no data)
                    self.inputs.append(s.split(":")[0])
            elif num == 5:
                key, value = "", b""
                for en, ew, ev in _fields(val):
                    if en == 1 and ew == 2:
                        key = bytes(ev).decode()
                    elif en == 2 and ew == 2:
                        value = ev
                self.attr[key] = value

    def attr_fields(self, key):
        return {num: val for num, _, val in _fields(self.attr.get(key, b""))}


def read_frozen_graph(path):
    """The layers of a frozen TF graph's dense ReLU chain, read from the protobuf wire format (no TF).

    Walks from ``output_layer/BiasAdd`` back to the ``input_layer`` placeholder through ``Identity`` nodes,
    accepting ``MatMul`` -> ``BiasAdd`` (-> ``Relu``) blocks only.  Returns a list of ``(W float32 (K, N),
    b float32 (N,))`` pairs, first layer first, whose ``relu`` attribute says which layers end in a ReLU.
    Anything else — another op, a dtype other than DT_FLOAT, ``transpose_a`` / ``transpose_b``, shapes that do
    not chain — raises ``ValueError`` naming the node."""
    if isinstance(path, (bytes, bytearray, memoryview)):
        data = bytes(path)
    else:
        with open(path, "rb") as f:
            data = f.read()
    nodes = {}
    for num, wt, val in _fields(memoryview(data)):
        if num == 1 and wt == 2:
            n = _Node(val)
            nodes[n.name] = n

    def get(name, seen=None):
        seen = seen or set()
        if name not in nodes:
            raise ValueError("node %r: not in the graph" % name)
        n = nodes[name]
        if n.op == "Identity":
            if name in seen or not n.inputs:
                raise ValueError("node %r: Identity without an input" % name)
            return get(n.inputs[0], seen | {name})
        return n

    def check_float(n):
        t = n.attr_fields("T")
        if 6 in t and t[6] != DT_FLOAT:
            raise ValueError("node %r: %s of dtype %d, not DT_FLOAT" % (n.name, n.op, t[6]))

    def const(name):
        n = get(name)
        if n.op != "Const":
            raise ValueError("node %r: %s where a Const was expected" % (n.name, n.op))
        d = n.attr_fields("dtype")
        if 6 in d and d[6] != DT_FLOAT:
            raise ValueError("node %r: Const of dtype %d, not DT_FLOAT" % (n.name, d[6]))
        v = n.attr_fields("value")
        if 8 not in v:
            raise ValueError("node %r: Const without a tensor value" % n.name)
        return _tensor(v[8], n.name)

    layers, relu = [], []
    n = get(OUTPUT_NAME)
    while True:
        if n.op == "Placeholder":
            if n.name != INPUT_NAME:
                raise ValueError("node %r: the chain starts at a placeholder other than %r" % (n.name, INPUT_NAME))
            d = n.attr_fields("dtype")
            if 6 in d and d[6] != DT_FLOAT:
                raise ValueError("node %r: placeholder of dtype %d, not DT_FLOAT" % (n.name, d[6]))
            break
        has_relu = n.op == "Relu"
        if has_relu:
            check_float(n)
            if len(n.inputs) != 1:
                raise ValueError("node %r: Relu needs one input" % n.name)
            n = get(n.inputs[0])
        if n.op != "BiasAdd":
            raise ValueError("node %r: unsupported op %s (MatMul, BiasAdd, Relu and Identity only)" % (n.name, n.op))
        check_float(n)
        if len(n.inputs) != 2:
            raise ValueError("node %r: BiasAdd needs two inputs" % n.name)
        b = const(n.inputs[1])
        mm = get(n.inputs[0])
        if mm.op != "MatMul":
            raise ValueError("node %r: unsupported op %s where a MatMul was expected" % (mm.name, mm.op))
        check_float(mm)
        for flag in ("transpose_a", "transpose_b"):
            if mm.attr_fields(flag).get(5, 0):
                raise ValueError("node %r: MatMul with %s" % (mm.name, flag))
        if len(mm.inputs) != 2:
            raise ValueError("node %r: MatMul needs two inputs" % mm.name)
        W = const(mm.inputs[1])
        if W.ndim != 2 or b.shape != (W.shape[1],):
            raise ValueError("node %r: weights %s and bias %s do not match" % (n.name, W.shape, b.shape))
        if layers and layers[0][0].shape[0] != W.shape[1]:
            raise ValueError("node %r: output width %d does not feed the next layer's %d inputs"
                             % (mm.name, W.shape[1], layers[0][0].shape[0]))
        layers.insert(0, (np.ascontiguousarray(W), np.ascontiguousarray(b)))
        relu.insert(0, has_relu)
        n = get(mm.inputs[0])
    if not layers:
        raise ValueError("node %r: no MatMul/BiasAdd layer between output and input" % OUTPUT_NAME)
    out = _Layers(layers)
    out.relu = tuple(relu)
    return out


class _Layers(list):
    """``read_frozen_graph``'s result: ``(W, b)`` pairs plus ``relu``, one bool per layer."""
    relu = ()


# ---------------------------------------------------------------- the network on the GPU
class Policy(_lib.Handle):
    """``Policy(graph_path)`` (scripts/policy.py:17-28) on the GPU.  ``predict_action(lidar)`` returns the
    steering angle of one scan as ``np.float32`` (the reference's ``sess.run(...)[0][0]``); ``predict_many``
    and ``predict_device`` evaluate batches in one launch.  The input window is ``scan[in_start : in_start +
    K]`` with ``x = r / scale if r <= clip else 1.0`` (policy.py:30,34)."""

    _destroy = "rl_policy_destroy"

    def __init__(self, graph_path=None, device=0, in_start=180, clip=15.0, scale=15.0, layers=None, relu=None):
        if layers is None:
            if graph_path is None:
                raise ValueError("Policy needs a graph path (or use Policy.from_arrays)")
            layers = read_frozen_graph(graph_path)
        if relu is None:
            relu = getattr(layers, "relu", None) or tuple(i < len(layers) - 1 for i in range(len(layers)))
        Ws = [np.ascontiguousarray(np.asarray(W, dtype=np.float32)) for W, _ in layers]
        bs = [np.ascontiguousarray(np.asarray(b, dtype=np.float32).reshape(-1)) for _, b in layers]
        if len(relu) != len(Ws) or not Ws:
            raise ValueError("one relu flag per layer, at least one layer")
        dims = [Ws[0].shape[0]] if Ws[0].ndim == 2 else [-1]
        for W, b in zip(Ws, bs):
            if W.ndim != 2 or W.shape[0] != dims[-1] or b.shape != (W.shape[1],):
                raise ValueError("layer shapes do not chain: %s" % [(w.shape, v.shape) for w, v in zip(Ws, bs)])
            dims.append(W.shape[1])
        self.layers = list(zip(Ws, bs))
        self.relu = tuple(bool(r) for r in relu)
        self.dims = tuple(int(d) for d in dims)
        self.in_start, self.clip, self.scale = int(in_start), float(clip), float(scale)
        self.device = int(device)
        self._h = C.c_void_p()
        _lib.call("rl_policy_create", self.device, len(Ws), np.array(self.dims, np.int32), Ws, bs,
                  np.array(self.relu, np.uint8), self.in_start, self.clip, self.scale, self._h)

    @classmethod
    def from_arrays(cls, layers, relu=None, device=0, in_start=180, clip=15.0, scale=15.0):
        """A policy from ``[(W (K, N), b (N,)), ...]``; ``relu`` defaults to every layer but the last."""
        return cls(None, device=device, in_start=in_start, clip=clip, scale=scale, layers=layers, relu=relu)

    @property
    def window(self):
        """(first beam, beams read) of each scan."""
        return self.in_start, self.dims[0]

    def predict_action(self, lidar):
        """Steering angle (np.float32) for one scan: ``Policy.predict_action(lidar)`` (policy.py:33-35)."""
        lidar = np.ascontiguousarray(np.asarray(lidar, dtype=np.float32).reshape(-1))
        return self.predict_many(lidar[None, :])[0]

    def predict_many(self, scans, size=None):
        """Steering angles float32 (n,) for scans float32 (n, size), or a flat (n*size,) array with ``size`` given
        (the layout ``scanMany`` returns)."""
        scans = np.asarray(scans)
        if scans.dtype != np.float32:
            raise ValueError("scans must be float32")
        scans = np.ascontiguousarray(scans)
        if scans.ndim == 2:
            n, size = scans.shape
        else:
            if not size or scans.size % int(size):
                raise ValueError("flat scans need a size that divides their length")
            size = int(size)
            n = scans.size // size
        out = np.empty(n, dtype=np.float32)
        _lib.call("rl_policy_eval", self, scans, n, size, out)
        return out

    def predict_device(self, d_scans_ptr, n_scans, size, d_steers_ptr, stream=0):
        """Device-resident form: ``d_scans_ptr`` -> float32[n_scans*size] (e.g. ``calc_range_fan_device``'s output),
        ``d_steers_ptr`` -> float32[n_scans]; asynchronous on ``stream``."""
        _lib.call("rl_policy_eval_device", self, int(d_scans_ptr), n_scans, size, int(d_steers_ptr), int(stream))
