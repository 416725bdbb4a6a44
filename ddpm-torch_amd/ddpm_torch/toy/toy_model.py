"""The toy denoiser of upstream ``ddpm_torch/toy/toy_model.py:17-62`` (``Decoder`` / ``TemporalLayer``) on the HIP kernels of
``csrc/toymlp.hip``.

The module keeps upstream's parameters and state-dict layout — one ``TemporalLayer`` object repeated ``num_temporal_layers`` times in
``temp_fc`` (so ``temp_fc.{1..L-1}.*`` alias ``temp_fc.0.*``) — and upstream's seeded initialisation (xavier-uniform weights in
construction order, zero biases, LayerNorm ones / zeros).  ``forward`` is ONE autograd node: the time table of all T timesteps and the
fused decoder forward (2 C-ABI calls), and in backward the fused row backward and the time-table backward (2 calls).  The time table is
recomputed from the live parameters on every call, so captured sampling steps and in-place optimiser updates never see a stale copy.
No CPU path: CPU tensors raise.
"""
import math

import torch
import torch.nn as nn

from .. import _hip
from ..functions import _freqs

__all__ = ["Decoder", "TemporalLayer"]

DEFAULT_T = 1000        # time-table rows when the caller gives no schedule length (covers every t upstream's toy configs draw)


class _Linear(nn.Module):
    """upstream ``modules.Linear``: weight [out][in] xavier-uniform (gain 1), bias zero; torch's own nn.Linear would draw a different init."""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty((out_features, in_features), dtype=torch.float32))
        if bias:
            self.bias = nn.Parameter(torch.empty((out_features,), dtype=torch.float32))
        else:
            self.register_parameter("bias", None)
        nn.init.xavier_uniform_(self.weight, gain=1.0)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, x):
        raise RuntimeError("the toy Decoder runs as one fused kernel; its sub-layers are not called on their own")

    def extra_repr(self):
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}"


class TemporalLayer(nn.Module):
    """toy_model.py:17-37 (skip = Identity: in == out == mid_features)."""

    def __init__(self, in_features, out_features, temporal_features):
        super().__init__()
        if in_features != out_features:
            raise NotImplementedError("the fused decoder serves in_features == out_features (the only form Decoder builds)")
        self.norm1 = nn.LayerNorm(in_features)
        self.fc1 = _Linear(in_features, out_features, bias=False)
        self.norm2 = nn.LayerNorm(out_features)
        self.fc2 = _Linear(out_features, out_features, bias=False)
        self.enc = _Linear(temporal_features, out_features)
        self.skip = nn.Identity()


class _TimeProj(nn.Sequential):
    def __init__(self, m):
        super().__init__(_Linear(m, m), nn.LeakyReLU(negative_slope=0.02, inplace=True))


def _ws_floats(B, D, M, L):
    r = lambda n: (n + 63) // 64 * 64
    K = L * B
    S = min(64, max(1, (K + 511) // 512))
    return 4 * r(K * M) + r(2 * S * M * M) + r(((B + 31) // 32) * (6 * M + 2 * M * D + D))


class _DecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t, want, T, D, M, L, *params):
        (w_in, n1w, n1b, fc1, n2w, n2b, fc2, encw, encb, onw, onb, outw, outb, tpw, tpb) = params
        B = x.shape[0]
        dev, s = x.device, _hip.stream()
        freqs = _freqs(M, dev)
        tabs = torch.empty(2 * T * M, dtype=torch.float32, device=dev)
        _hip.call("ddpm_toy_time_table", freqs.data_ptr(), tpw.data_ptr(), tpb.data_ptr(), encw.data_ptr(), encb.data_ptr(), tabs.data_ptr(),
                  T, M, s)
        y = torch.empty((B, D), dtype=torch.float32, device=dev)
        saved = torch.empty((L + 1) * B * M + B * (2 * L + 1) * 2, dtype=torch.float32, device=dev) if want else None
        _hip.call("ddpm_toy_decoder_fwd", x.data_ptr(), t.data_ptr(), *[p.data_ptr() for p in (w_in, n1w, n1b, fc1, n2w, n2b, fc2, onw, onb, outw, outb)],
                  tabs.data_ptr(), y.data_ptr(), _hip.ptr(saved), B, D, M, L, T, s)
        if want:
            ctx.save_for_backward(x, t, tabs, saved, *params)
            ctx.geom = (T, D, M, L)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, t, tabs, saved, *params = ctx.saved_tensors
        (w_in, n1w, n1b, fc1, n2w, n2b, fc2, encw, encb, onw, onb, outw, outb, tpw, tpb) = params
        T, D, M, L = ctx.geom
        B, dev, s = x.shape[0], x.device, _hip.stream()
        gy = gy.contiguous().float()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        MD, MM = M * D, M * M
        gdec = torch.empty(2 * MD + 6 * M + 2 * MM + D, dtype=torch.float32, device=dev)
        gtab = torch.empty(2 * MM + 2 * M, dtype=torch.float32, device=dev)
        dzsum = torch.empty(B * M, dtype=torch.float32, device=dev)
        nws = max(_ws_floats(B, D, M, L), 3 * T * M)
        ws = torch.empty(nws, dtype=torch.float32, device=dev)
        _hip.call("ddpm_toy_decoder_bwd", x.data_ptr(), t.data_ptr(), gy.data_ptr(),
                  *[p.data_ptr() for p in (w_in, n1w, n1b, fc1, n2w, n2b, fc2, onw, onb, outw)], tabs.data_ptr(), saved.data_ptr(),
                  _hip.ptr(dx), gdec.data_ptr(), dzsum.data_ptr(), ws.data_ptr(), nws, B, D, M, L, T, s)
        _hip.call("ddpm_toy_time_table_bwd", t.data_ptr(), dzsum.data_ptr(), _freqs(M, dev).data_ptr(), encw.data_ptr(), tabs.data_ptr(),
                  gtab.data_ptr(), ws.data_ptr(), nws, B, M, T, s)
        sizes = [MD, M, M, MM, M, M, MM, M, M, MD, D]
        g_in, g_n1w, g_n1b, g_fc1, g_n2w, g_n2b, g_fc2, g_onw, g_onb, g_outw, g_outb = gdec.split(sizes)
        g_encw, g_encb, g_tpw, g_tpb = gtab.split([MM, M, MM, M])
        grads = [g_in, g_n1w, g_n1b, g_fc1, g_n2w, g_n2b, g_fc2, g_encw, g_encb, g_onw, g_onb, g_outw, g_outb, g_tpw, g_tpb]
        grads = [g.view_as(p) for g, p in zip(grads, params)]
        return (dx, None, None, None, None, None, None, *grads)


class Decoder(nn.Module):
    """toy_model.py:40-62: ``Decoder(in_features, mid_features, num_temporal_layers)``; ``forward(x [B, D], t [B] int64) -> [B, D]``.

    ``timesteps`` (not in upstream) is the number of rows of the time table: t must lie in [0, timesteps).  The toy
    ``GaussianDiffusion`` sets it to its schedule length before every call; the default covers T <= 1000."""

    def __init__(self, in_features, mid_features, num_temporal_layers):
        super().__init__()
        if not (1 <= in_features <= 16 and mid_features % 32 == 0 and 32 <= mid_features <= 256 and num_temporal_layers >= 1):
            raise ValueError("the fused toy decoder serves 1 <= in_features <= 16, mid_features in 32..256 (a multiple of 32), "
                             "num_temporal_layers >= 1")
        self.in_fc = _Linear(in_features, mid_features, bias=False)
        self.temp_fc = nn.Sequential(*([TemporalLayer(mid_features, mid_features, mid_features)] * num_temporal_layers))
        self.out_norm = nn.LayerNorm(mid_features)
        self.out_fc = _Linear(mid_features, in_features)
        self.t_proj = _TimeProj(mid_features)
        self.in_features, self.mid_features, self.num_temporal_layers = in_features, mid_features, num_temporal_layers
        self.timesteps = DEFAULT_T

    def _params(self):
        lay = self.temp_fc[0]
        return (self.in_fc.weight, lay.norm1.weight, lay.norm1.bias, lay.fc1.weight, lay.norm2.weight, lay.norm2.bias, lay.fc2.weight,
                lay.enc.weight, lay.enc.bias, self.out_norm.weight, self.out_norm.bias, self.out_fc.weight, self.out_fc.bias,
                self.t_proj[0].weight, self.t_proj[0].bias)

    def forward(self, x, t):
        params = self._params()
        _hip.require_cuda(x, t, *params)
        if any(p.dtype != torch.float32 for p in params):
            raise TypeError("the toy decoder is fp32 only")
        if x.ndim != 2 or x.shape[1] != self.in_features or t.shape != (x.shape[0],):
            raise ValueError(f"expected x [B, {self.in_features}] and t [B]; got {tuple(x.shape)} and {tuple(t.shape)}")
        x = x.contiguous().float()
        t = t.to(torch.int64).contiguous()
        params = tuple(p if p.is_contiguous() else p.contiguous() for p in params)
        want = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
        return _DecoderFn.apply(x, t, want, int(self.timesteps), self.in_features, self.mid_features, self.num_temporal_layers, *params)
