"""Shared by tests/test_autoclip_abi.py (CPU) and tests/test_gpu_autoclip_device.py: the sequences of gradient norms the device
form of AutoClip is fed one by one, a driver of the host twin (ops.autoclip_observe_host) with the class's ping-pong and growth,
and the byte comparison (NaN equals NaN of the same bits).  Everything is seeded; nothing here needs a GPU."""
import numpy as np
import torch

PERCENTILES = (0, 37.5, 50, 100)
OUT_DOUBLES = 4                # ops.AUTOCLIP_OUT_DOUBLES
SCALE_F32_INDEX = 6            # ops.AUTOCLIP_SCALE_F32_INDEX


def sequences():
    """{name: float64 array}: every entry a norm (>= +0, +inf or NaN)"""
    rng = np.random.default_rng(20240607)
    nan_at_5 = rng.lognormal(0.0, 1.0, 12)
    nan_at_5[5] = np.nan
    one_inf = rng.lognormal(0.0, 1.0, 9)
    one_inf[3] = np.inf
    two_inf = rng.lognormal(0.0, 1.0, 9)
    two_inf[2] = two_inf[6] = np.inf
    return {
        "ascending": np.arange(1, 14, dtype=np.float64) * 0.37,
        "descending": (np.arange(13, 0, -1, dtype=np.float64)) * 0.61,            # every insert lands at the head
        "constant": np.full(11, 2.5),                                              # all ties
        "lognormal": rng.lognormal(0.0, 1.5, 24),
        "one_inf": one_inf,
        "two_inf": two_inf,
        "one_then_inf": np.array([1.0, np.inf]),                                  # at 50: inf - inf * 0.5 = NaN in numpy
        "nan_at_5": nan_at_5,
        "len1": np.array([0.8125]),
        "len2": np.array([3.0, 0.0]),
        "len3": np.array([2.0, 7.0, 2.0]),
    }


def branch_of(n, q):
    """which branch of `t >= 0.5` the step with n held norms takes at percentile q"""
    vi = n * (q / 100.0)
    return (vi - np.floor(vi)) >= 0.5


def bits(x):
    """bytes of a tensor / array / float, so that NaN equals NaN (of the same bits) and -0 differs from +0"""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x)).tobytes()


class HostClip(object):
    """the host twin (device="cpu") or the kernels (device="cuda") driven as dcl.optim.DeviceAutoClip drives them: two sorted
    buffers used in turn, an arrival buffer, all three doubling from `capacity`; every buffer is prefilled with NaN so that a
    write beyond the n + 1 entries shows"""

    def __init__(self, ops, percentile, capacity=2, device="cpu"):
        self.ops, self.percentile, self.capacity, self.n, self.device = ops, percentile, capacity, 0, device
        self.fn = ops.autoclip_observe_host if device == "cpu" else ops.autoclip_observe
        self.sorted = [self._new(capacity), self._new(capacity)]
        self.arrival = self._new(capacity)
        self.out = torch.zeros(OUT_DOUBLES, dtype=torch.float64, device=device)
        self.grown = 0

    def _new(self, k):
        return torch.full((k,), float("nan"), dtype=torch.float64, device=self.device)

    def observe(self, x):
        if self.n == self.capacity:
            self.capacity *= 2
            self.grown += 1
            src, arr = self.sorted[0], self.arrival
            self.sorted, self.arrival = [self._new(self.capacity), self._new(self.capacity)], self._new(self.capacity)
            self.sorted[0][:self.n] = src[:self.n]
            self.arrival[:self.n] = arr[:self.n]
        src, dst = self.sorted
        norm = torch.from_numpy(np.array([x], dtype=np.float64)).to(self.device)
        self.fn(self.n, src, dst, self.arrival, norm, self.percentile, self.out)
        self.sorted = [dst, src]
        self.n += 1
        return self

    def everything(self):
        """the bytes of all four outputs, the untouched rest of the buffers included"""
        return bits(self.sorted[0]), bits(self.arrival), bits(self.out)

    @property
    def held(self):
        return self.sorted[0][:self.n].cpu().numpy()

    @property
    def beyond(self):
        return self.sorted[0][self.n:].cpu().numpy()

    @property
    def clip_value(self):
        return float(self.out[1])

    @property
    def scale(self):
        return float(self.out[2])

    @property
    def scale32(self):
        return self.out.view(torch.float32)[SCALE_F32_INDEX].cpu().numpy()
