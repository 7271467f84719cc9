"""Policy populations on the GPU (include/scanlib_population.h): N steering networks of one architecture evaluated in
one launch and driven in one closed loop — what evolution strategies, CMA-ES, population-based search and the scoring
of a directory of checkpoints need of ``policy.Policy``.

A member is one flat float32 parameter vector θ of ``n_params`` values: for every layer ``W`` (K, N) row-major, then
``b`` (N,) (``pack`` / ``unpack``).  Scan row i of a call with ``cars_per_member`` = E is answered by member
``first + i // E``, bit for bit as ``Policy.from_arrays(unpack(θ))`` answers it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def n_params(dims):
    """P = Σ (dims[l] + 1) · dims[l + 1]."""
    return sum((int(dims[l]) + 1) * int(dims[l + 1]) for l in range(len(dims) - 1))


def pack(layers):
    """``[(W (K, N), b (N,)), ...]`` -> θ float32 (P,): every layer's ``W`` row-major, then its ``b``."""
    parts = []
    for W, b in layers:
        W, b = np.asarray(W, np.float32), np.asarray(b, np.float32).reshape(-1)
        if W.ndim != 2 or b.shape != (W.shape[1],) or (parts and parts[-1].size != W.shape[0]):
            raise ValueError("layer shapes do not chain: %s" % [(np.shape(w), np.shape(v)) for w, v in layers])
        parts += [W.reshape(-1), b]
    if not parts:
        raise ValueError("at least one layer")
    return np.concatenate(parts)


def unpack(theta, dims):
    """θ float32 (P,) -> ``[(W (dims[l], dims[l + 1]), b (dims[l + 1],)), ...]`` (copies)."""
    theta = np.asarray(theta)
    if theta.dtype != np.float32 or theta.shape != (n_params(dims),):
        raise ValueError("theta must be float32 (%d,) for dims %s" % (n_params(dims), tuple(dims)))
    layers, o = [], 0
    for l in range(len(dims) - 1):
        K, N = int(dims[l]), int(dims[l + 1])
        layers.append((theta[o:o + K * N].reshape(K, N).copy(), theta[o + K * N:o + (K + 1) * N].copy()))
        o += (K + 1) * N
    return layers


class PolicyPopulation(_lib.Handle):
    """``n_members`` networks of the architecture ``dims`` (``(720, 64, 128, 128, 64, 1)`` is the reference's), all
    zero until set.  ``relu`` defaults to every layer but the last; ``in_start``, ``clip`` and ``scale`` as ``Policy``
    takes them."""

    _destroy = "rl_policy_pop_destroy"

    def __init__(self, dims, n_members, relu=None, device=0, in_start=180, clip=15.0, scale=15.0):
        dims = tuple(int(d) for d in dims)
        if len(dims) < 2:
            raise ValueError("dims needs an input width and at least one layer")
        if relu is None:
            relu = tuple(i < len(dims) - 2 for i in range(len(dims) - 1))
        if len(relu) != len(dims) - 1:
            raise ValueError("one relu flag per layer")
        if int(n_members) < 1:
            raise ValueError("n_members must be >= 1")
        self.dims, self.relu = dims, tuple(bool(r) for r in relu)
        self.n_members, self.n_params = int(n_members), n_params(dims)
        self.in_start, self.clip, self.scale = int(in_start), float(clip), float(scale)
        self.device = int(device)
        self._h = C.c_void_p()
        _lib.call("rl_policy_pop_create", self.device, self.n_members, len(dims) - 1, np.array(dims, np.int32),
                  np.array(self.relu, np.uint8), self.in_start, self.clip, self.scale, self._h)
        n, p = C.c_int(), C.c_int()
        _lib.call("rl_policy_pop_layout", self, n, p)
        assert (n.value, p.value) == (self.n_members, self.n_params)

    @classmethod
    def from_policies(cls, policies, device=None):
        """A population whose member m is ``policies[m]`` (``Policy`` objects of one architecture, window and ReLU
        pattern)."""
        policies = list(policies)
        if not policies:
            raise ValueError("at least one policy")
        p0 = policies[0]
        key = (p0.dims, p0.relu, p0.in_start, p0.clip, p0.scale)
        for p in policies[1:]:
            if (p.dims, p.relu, p.in_start, p.clip, p.scale) != key:
                raise ValueError("the policies of a population share one architecture, window and input transform")
        pop = cls(p0.dims, len(policies), relu=p0.relu, device=p0.device if device is None else device,
                  in_start=p0.in_start, clip=p0.clip, scale=p0.scale)
        pop.set(np.stack([pack(p.layers) for p in policies]))
        return pop

    @property
    def window(self):
        """(first beam, beams read) of each scan."""
        return self.in_start, self.dims[0]

    def _range(self, first, n):
        first = int(first)
        n = self.n_members - first if n is None else int(n)
        if first < 0 or n < 0 or first + n > self.n_members:
            raise ValueError("members [%d, %d) do not lie in [0, %d)" % (first, first + n, self.n_members))
        return first, n

    def set(self, theta, first=0):
        """Members ``first ...`` from θ float32 (n, P) (or (P,) for one); synchronous."""
        theta = np.asarray(theta)
        if theta.ndim == 1:
            theta = theta[None, :]
        if theta.dtype != np.float32 or theta.ndim != 2 or theta.shape[1] != self.n_params:
            raise ValueError("theta must be float32 (n, %d)" % self.n_params)
        first, n = self._range(first, theta.shape[0])
        _lib.call("rl_policy_pop_set", self, first, n, np.ascontiguousarray(theta))

    def set_device(self, tensor, first=0):
        """Members ``first ...`` from a contiguous float32 torch tensor (n, P) on this handle's device; enqueued on
        ``torch.cuda.current_stream()``, nothing waits."""
        import torch
        if not isinstance(tensor, torch.Tensor) or tensor.dtype != torch.float32 or not tensor.is_contiguous():
            raise ValueError("theta must be a contiguous float32 torch tensor")
        if tensor.dim() == 1:
            tensor = tensor[None, :]
        if tensor.dim() != 2 or tensor.shape[1] != self.n_params:
            raise ValueError("theta must be (n, %d)" % self.n_params)
        if tensor.device.type != "cuda" or tensor.device.index != self.device:
            raise ValueError("theta must live on cuda:%d (got %s)" % (self.device, tensor.device))
        first, n = self._range(first, tensor.shape[0])
        stream = torch.cuda.current_stream(tensor.device).cuda_stream
        _lib.call("rl_policy_pop_set_device", self, first, n, int(tensor.data_ptr()), int(stream))

    def get(self, m):
        """θ float32 (P,) of member ``m``, the bits that were set."""
        m, _ = self._range(m, 1)
        out = np.empty(self.n_params, np.float32)
        _lib.call("rl_policy_pop_get", self, m, out)
        return out

    def member(self, m):
        """Member ``m`` as a ``Policy`` of its own (a copy of its θ)."""
        from .policy import Policy
        return Policy.from_arrays(unpack(self.get(m), self.dims), self.relu, device=self.device,
                                  in_start=self.in_start, clip=self.clip, scale=self.scale)

    def predict_many(self, scans, cars_per_member, first=0, n=None):
        """Steers float32 (n E,) of scans float32 (n E, size): row i by member ``first + i // E``, E =
        ``cars_per_member``; ``n`` defaults to the members from ``first`` on."""
        scans = np.asarray(scans)
        if scans.dtype != np.float32 or scans.ndim != 2:
            raise ValueError("scans must be float32 (n * cars_per_member, size)")
        E = int(cars_per_member)
        if E < 1:
            raise ValueError("cars_per_member must be >= 1")
        first, n = self._range(first, scans.shape[0] // E if n is None else n)
        if scans.shape[0] != n * E:
            raise ValueError("scans must hold %d members x %d cars = %d rows (got %d)" % (n, E, n * E, scans.shape[0]))
        if scans.shape[1] < self.in_start + self.dims[0]:
            raise ValueError("scans of %d beams do not hold the policy's window [%d, %d)"
                             % (scans.shape[1], self.in_start, self.in_start + self.dims[0]))
        out = np.empty(n * E, np.float32)
        _lib.call("rl_policy_pop_eval", self, first, n, E, np.ascontiguousarray(scans), scans.shape[1], out)
        return out

    def predict_rows(self, scans, members, out=None):
        """Row-indexed evaluation (``rl_policy_pop_eval_rows``, include/scanlib_league.h): steers float32 (n,) of scans
        float32 (n, size), row i by member ``members[i]``, in any order.  A row with ``members[i] == -1`` is not
        answered: it keeps the value ``out`` (float32 (n,), written in place when C-contiguous) holds there, NaN
        without ``out``."""
        from .league import member_args
        scans = np.asarray(scans)
        if scans.dtype != np.float32 or scans.ndim != 2:
            raise ValueError("scans must be float32 (n, size)")
        n = scans.shape[0]
        members = member_args(members, n, self.n_members)
        if scans.shape[1] < self.in_start + self.dims[0]:
            raise ValueError("scans of %d beams do not hold the policy's window [%d, %d)"
                             % (scans.shape[1], self.in_start, self.in_start + self.dims[0]))
        if out is None:
            out = np.full(n, np.nan, np.float32)
        else:
            out = np.asarray(out)
            if out.dtype != np.float32 or out.shape != (n,):
                raise ValueError("out must be float32 (%d,)" % n)
            out = np.ascontiguousarray(out)
        _lib.call("rl_policy_pop_eval_rows", self, n, members, np.ascontiguousarray(scans), scans.shape[1], out)
        return out

    def predict_rows_device(self, d_scans_ptr, d_members_ptr, n, size, d_steers_ptr, stream=0):
        """Device-resident form of ``predict_rows``: ``d_scans_ptr`` -> float32[n size], ``d_members_ptr`` -> int32[n],
        ``d_steers_ptr`` -> float32[n]; asynchronous on ``stream``.  An entry outside [0, n_members) is treated as -1."""
        n, size = int(n), int(size)
        if n < 0:
            raise ValueError("n must be >= 0")
        if size < self.in_start + self.dims[0]:
            raise ValueError("scans of %d beams do not hold the policy's window [%d, %d)"
                             % (size, self.in_start, self.in_start + self.dims[0]))
        _lib.call("rl_policy_pop_eval_rows_device", self, n, int(d_members_ptr), int(d_scans_ptr), size,
                  int(d_steers_ptr), int(stream))

    def predict_device(self, d_scans_ptr, cars_per_member, size, d_steers_ptr, first=0, n=None, stream=0):
        """Device-resident form: ``d_scans_ptr`` -> float32[n E size], ``d_steers_ptr`` -> float32[n E];
        asynchronous on ``stream``."""
        first, n = self._range(first, n)
        _lib.call("rl_policy_pop_eval_device", self, first, n, int(cars_per_member), int(d_scans_ptr), int(size),
                  int(d_steers_ptr), int(stream))
