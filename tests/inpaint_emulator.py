"""TEST INFRASTRUCTURE for inpainting and image editing (csrc/inpaint.hip, GaussianDiffusion.inpaint / edit): numpy restatements of
``ddpm_p_sample_step_masked`` and ``ddpm_q_jump`` as include/ddpm_hip.h states them, over the raw host pointers the product passes, for the
host emulator (tests/abi_emulator.py; ``attach`` hangs them on the Emulator instance ``install`` returns).  The reverse-step half of the
masked step IS the emulator's own ``ddpm_p_sample_step`` (rows of n floats) or tests/learned_var_emulator.py's ``ddpm_p_sample_step_lv``
(rows of 2n floats), so an element the mask leaves to the reverse step carries their bits, as the header promises of the kernels.  fp32
arithmetic like the kernels'; they say nothing about the kernels themselves — tests/test_inpaint_gpu.py holds those to float64."""
import numpy as np

from tests import learned_var_emulator as LV
from tests.abi_emulator import f32, i64

NAN = np.float32("nan")


def _times(t, B, T):
    tt = i64(t, B)
    return np.clip(tt, 0, T - 1).astype(np.int64), (tt >= 0) & (tt < T)


def masked_step(emu, x_t, out, z, x_known, e, mask, t, recip, recip_m1, c1, c2, lo, hi, ka, kb, x_prev, B, n, hw, mask_rows, pitch, mean_type, clip,
                var_mode, T, st):
    assert x_t and out and z and x_known and e and mask and t and recip and recip_m1 and c1 and c2 and ka and kb and x_prev
    assert 0 < B <= 65535 and n > 0 and hw > 0 and T > 0 and n % hw == 0 and mask_rows in (1, B) and pitch in (n, 2 * n)
    assert 0 <= mean_type <= 2 and 0 <= var_mode <= 2 and (var_mode == 0 or pitch == 2 * n) and (var_mode == 1 or lo) and (var_mode != 2 or hi)
    tc, ok = _times(t, B, T)
    u = np.full((B, n), NAN, dtype=np.float32)
    with np.errstate(all="ignore"):
        if pitch == n:
            emu.ddpm_p_sample_step(x_t, out, z, tc.ctypes.data, recip, recip_m1, c1, c2, lo, u.ctypes.data, 0, B, n, mean_type, clip, T, st)
        else:
            LV.ddpm_p_sample_step_lv(x_t, out, z, tc.ctypes.data, recip, recip_m1, c1, c2, lo, hi, u.ctypes.data, 0, B, n, mean_type, clip, var_mode, T, st)
        a, b = f32(ka, T)[tc][:, None], f32(kb, T)[tc][:, None]
        k = a * f32(x_known, B * n).reshape(B, n) + b * f32(e, B * n).reshape(B, n)
        m = np.broadcast_to(np.tile(f32(mask, mask_rows * hw).reshape(mask_rows, hw), (1, n // hw)), (B, n))
        mix = m * k + (np.float32(1.0) - m) * u
    val = np.where(m == 0, u, np.where(m == 1, k, mix))
    f32(x_prev, B * n).reshape(B, n)[...] = np.where(ok[:, None], val, NAN)                 # (u was formed from copies: x_prev may be x_t)


def q_jump(x, z, t, ja, jb, x_out, B, n, T, st):
    assert x and z and t and ja and jb and x_out and 0 < B <= 65535 and n > 0 and T > 0
    tc, ok = _times(t, B, T)
    with np.errstate(all="ignore"):
        val = f32(ja, T)[tc][:, None] * f32(x, B * n).reshape(B, n) + f32(jb, T)[tc][:, None] * f32(z, B * n).reshape(B, n)
    f32(x_out, B * n).reshape(B, n)[...] = np.where(ok[:, None], val, NAN)


def attach(emu):
    """Add the two entry points to an ``abi_emulator.Emulator`` instance (its ``call`` is ``getattr(self, name)``); the 2n-row reverse
    step comes with them (tests/learned_var_emulator.py)."""
    LV.attach(emu)
    emu.masked_args = []                                    # (B, n, hw, mask_rows, out_pitch, mean_type, clip, var_mode, T) of every call

    def logged(*a):
        emu.masked_args.append(tuple(a[16:25]))
        masked_step(emu, *a)

    emu.ddpm_p_sample_step_masked = logged
    emu.ddpm_q_jump = q_jump
    return emu
