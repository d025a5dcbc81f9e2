"""CPU evidence for tests/test_gpu_vision_f32_bwd_frames.py: k_vision_bwd_f32's arithmetic
(csrc/vision_bwd_f32.h) emulated in torch at that test's shapes -- every fp32 operand split into
hi / mid / lo bf16 parts (gemm.h split3_bf16), the products of each k step of 16 in the kernel's
order (SPLIT6: lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi; conv1's weight gradient lo, mid, hi
against the exact image), fp32 accumulation, the K order per frame, a workgroup's accumulators carried
across its frames, the partials summed as k_vbwd_reduce does -- stays within the GPU test's bounds
(e2 / 2 of each live site, tests/f32_split_ref.py), so the bounds are reachable before GPU time is
spent.  Plus host checks of the index functions the kernel adds, and the entry's refusals."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f32_split_ref as R
from helpers import assert_close, detinit, rel_err

import attention

N = attention._pkg._native
PARAMS = detinit.deterministic_params(0, 18)
RTOL = 1e-4   # tests/test_gpu_parity.py RTOL (importing that module needs no GPU either, but drags the agent in)
SITES = {"dy1": ("dgrad2.W", "dgrad2.dy2"), "gW2": ("wgrad2.y1", "wgrad2.dy2"), "gW1": ("wgrad1.dy1",)}
ORDER6 = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))   # (A part, B part), smallest first


def split3(x):
    """(3, ...) fp32: the hi / mid / lo bf16 parts of fp32 x, as fp32."""
    hi = x.to(torch.bfloat16).float()
    r = x - hi
    mid = r.to(torch.bfloat16).float()
    lo = (r - mid).to(torch.bfloat16).float()
    return torch.stack([hi, mid, lo])


def _nhwc(t):
    return t.permute(0, 3, 2, 1).contiguous()   # (N, H, W, C) <-> the reference's (N, C, W, H)


def _mma(acc, A, B, order):
    """acc (M, N) += the products of A parts (3, K, M)^T and B parts (3, K, N), 16 k at a time, fp32."""
    for k0 in range(0, A.shape[1], 16):
        for qa, qb in order:
            acc += A[qa, k0:k0 + 16].t() @ B[qb, k0:k0 + 16]
    return acc


def _pad_rows(x, rows):
    return torch.cat([x, torch.zeros(x.shape[0], rows - x.shape[1], x.shape[2])], 1)


def emulate(frames, y1, dy2, groups):
    """frames (n,H,W,3) uint8, y1 (n,H1,W1,32) fp32, dy2 (n,h*w,64) fp32 -> packed gW2 [64][512], gW1 [32][256], gb1,
    dy1 (n,H1,W1,32), as ``groups`` workgroups (frame f on workgroup f % groups) and the reduce launch give them."""
    n, H, W, _ = frames.shape
    _, H1, W1, _ = y1.shape
    h, w = R.ref_cpu.grid_of(H, W)
    P, P1, Ha, Wa = h * w, H1 * W1, (H1 + 1) // 2, (W1 + 1) // 2
    w2 = torch.as_tensor(np.ascontiguousarray(PARAMS[R.CNN + "1.weight"])).float()   # (64, 32, kx, ky)
    # k_WdT2: W_c[ci][(ty*2+tx)*64 + co] = W2[co][ci][kx][ky], ky = py + 2(1-ty), kx = px + 2(1-tx)
    Wc = torch.zeros(4, 32, 256)
    for cls in range(4):
        for t in range(4):
            ky, kx = (cls >> 1) + 2 * (1 - (t >> 1)), (cls & 1) + 2 * (1 - (t & 1))
            Wc[cls, :, t * 64:(t + 1) * 64] = w2[:, :, kx, ky].t()
    Wcs = split3(Wc)                                           # (3, 4, 32, 256)
    parts = []
    dy1_all = torch.zeros(n, H1, W1, 32)
    for g in range(groups):
        acc2, acc1, bsum = torch.zeros(64, 512), torch.zeros(32, 256), torch.zeros(32)
        for f in range(g, n, groups):
            d = split3(dy2[f])                                 # (3, P, 64)
            yp = F.pad(split3(y1[f]), (0, 0, 2, 2, 2, 2))      # (3, H1+4, W1+4, 32)
            # conv2 wgrad: B row pix = the 4x4 window at (2 y2, 2 x2), columns (ky*4+kx)*32 + ci
            win = yp.unfold(1, 4, 2).unfold(2, 4, 2)           # (3, h', w', 32, ky, kx)
            B = win[:, :h, :w].permute(0, 1, 2, 4, 5, 3).reshape(3, P, 512)
            _mma(acc2, _pad_rows(d, 128), _pad_rows(B, 128), ORDER6)
            # conv2 dgrad by parity class: column n = a * Wa + b reads dY2 pixel (a + ty, b + tx) of tap t
            dg = F.pad(d.reshape(3, h, w, 64), (0, 0, 0, Wa + 1 - w, 0, Ha + 1 - h))   # zero pixels off the grid
            dy1 = torch.zeros(H1, W1, 32)
            for cls in range(4):
                py, px = cls >> 1, cls & 1
                G = torch.cat([dg[:, (t >> 1):(t >> 1) + Ha, (t & 1):(t & 1) + Wa] for t in range(4)], 3)
                G = G.reshape(3, Ha * Wa, 256).permute(0, 2, 1).contiguous()            # (3, K 256, NA)
                A = Wcs[:, cls].permute(0, 2, 1).contiguous()                            # (3, K 256, 32)
                acc = _mma(torch.zeros(32, Ha * Wa), A, G, ORDER6).t().reshape(Ha, Wa, 32)
                ny, nx = (H1 - py + 1) // 2, (W1 - px + 1) // 2
                dy1[py::2, px::2] = acc[:ny, :nx]
            bsum += dy1.reshape(P1, 32).sum(0)
            dy1_all[f] = dy1
            # conv1 wgrad: dY1 in three parts against the exact bf16 image, K = P1 padded to 16
            xp = F.pad(frames[f].float(), (0, 1, 1, 1, 1, 1))  # (H+2, W+2, 4)
            xw = xp.unfold(0, 8, 4).unfold(1, 8, 4)            # (H1', W1', 4, ky, kx)
            X = xw[:H1, :W1].permute(0, 1, 3, 4, 2).reshape(1, P1, 256)
            K1 = (P1 + 15) // 16 * 16
            _mma(acc1, _pad_rows(split3(dy1.reshape(P1, 32)), K1), _pad_rows(X, K1), ((2, 0), (1, 0), (0, 0)))
        parts.append(torch.cat([acc2.reshape(-1), acc1.reshape(-1), bsum]))
    part = torch.stack(parts)
    q = [part[groups * i // 4:groups * (i + 1) // 4].cumsum(0)[-1] if groups * (i + 1) // 4 > groups * i // 4
         else torch.zeros(part.shape[1]) for i in range(4)]
    tot = ((q[0] + q[1]) + q[2]) + q[3]
    return tot[:32768].reshape(64, 512), tot[32768:40960].reshape(32, 256), tot[40960:], dy1_all


CASES = {"2x84x84": (2, 84, 84, 2), "5x64x64": (5, 64, 64, 5), "5x84x84-groups2": (5, 84, 84, 2)}


@pytest.mark.parametrize("case", list(CASES))
def test_emulated_kernel_meets_the_gpu_bounds(case):
    n, H, W, groups = CASES[case]
    h, w = R.ref_cpu.grid_of(H, W)
    fr = torch.from_numpy(detinit.frames_u8(1234, (1, n, H, W, 3)))[0]
    dy2 = R.rnd((n, h * w, 64), 7)
    w1, b1, w2, b2 = R.cnn_weights(PARAMS, torch.float32)
    y1 = _nhwc(F.conv2d(_nhwc(fr.float()), w1, b1, stride=4, padding=1))   # (n, H1, W1, 32): an fp32 forward's Y1
    gW2p, gW1p, gb1, dy1 = emulate(fr, y1, dy2, groups)
    got = {"gW2": gW2p.reshape(64, 4, 4, 32).permute(0, 3, 2, 1), "dy1": _nhwc(dy1),
           "gW1": gW1p.reshape(32, 8, 8, 4)[..., :3].permute(0, 3, 2, 1)}
    assert float(gW1p.reshape(32, 8, 8, 4)[..., 3].abs().max()) == 0.0   # the image's fourth channel is zero
    ex, e2 = R.cnn_e2(R.cnn_weights(PARAMS), _nhwc(fr.float()), _nhwc(dy2.reshape(n, h, w, 64)), _nhwc(y1), _nhwc(dy1))
    bad = []
    for obs, sites in SITES.items():
        err = rel_err(got[obs], ex[obs])
        for s in sites:
            print(f"{case}: {obs} err {err:.3e}, e2[{s}] {e2[s, obs]:.3e}, err / e2 {err / e2[s, obs]:.3f}")
            if not err <= e2[s, obs] / 2:
                bad.append((case, obs, s, err, e2[s, obs]))
    assert not bad, bad
    assert_close(gb1.numpy(), ex["gb1"].numpy(), RTOL, f"{case}: gb1")


# ------------------------------------------------------------ index functions ----
D_PLANE, Y_PLANE, T_PLANE, X_IMG = 128 * 128, 36864, 416 * 64, 59392   # vision_bwd.h / vision.h byte sizes
Y_OFF, LDS = 3 * D_PLANE, 3 * D_PLANE + 3 * Y_PLANE
T_OFF = LDS - 3 * T_PLANE


def vb_dofs(pix, ch):
    """vision_bwd.h vb_dofs: 16-B chunk ch / 8 of dY2 pixel pix sits at slot (ch / 8) ^ ((pix / 2) % 8)."""
    return pix * 128 + ((((ch >> 3) ^ (pix >> 1)) & 7) << 4) + (ch & 7) * 2


def test_lds_phases_fit():
    assert LDS == 159744 and LDS <= 160 * 1024           # phase 1: dY2 + Y1 planes
    assert T_OFF == 79872 and T_OFF >= 3 * D_PLANE       # phase 2: dY1 planes clear of the dY2 planes
    assert X_IMG <= T_OFF                                # phase 3: the image clear of the dY1 planes
    for H, W in ((84, 84), (64, 64)):
        H1, W1 = (H + 2 - 8) // 4 + 1, (W + 2 - 8) // 4 + 1
        h, w = R.ref_cpu.grid_of(H, W)
        assert (H1 + 4) * (W1 + 4) * 64 <= Y_PLANE and H1 * W1 <= 416 and h * w <= 127 and (H + 2) * (W + 2) * 8 <= X_IMG
        assert h * w * 64 <= 8 * 256 * 4 and H1 * W1 * 32 <= 13 * 256 * 4 and W1 >= 8   # the register prefetch slots
        # the farthest Y1 pixel conv2's weight gradient reads, and the farthest image pixel conv1's does
        assert (2 * (h - 1) + 3) * (W1 + 4) + 2 * (w - 1) + 3 < (H1 + 4) * (W1 + 4)
        assert 4 * (H1 - 1) + 7 <= H + 1 and 4 * (W1 - 1) + 7 <= W + 1


def test_dy2_plane_offsets_are_a_bijection():
    offs = sorted(vb_dofs(p, c) for p in range(128) for c in range(0, 64, 4))
    assert offs == list(range(0, D_PLANE, 8))            # every 8-B piece of the plane exactly once
    for p in range(0, 128, 16):                          # 16 consecutive pixels, one chunk: 8 bank groups twice
        assert sorted((vb_dofs(p + i, 8) >> 4) & 7 for i in range(16)) == sorted(list(range(8)) * 2)


def test_presplit_fragment_order():
    """misc.hip vis_split_el at 128 rows, nks 16: the 16-B fragment of (row, k) is the one lane
    (k / 8 % 2) * 32 + row % 32 of wave row / 32 reads at k step k / 16 -- a bijection onto the region."""
    seen = set()
    for row in range(128):
        for k in range(256):
            frag = ((row >> 5) * 16 + (k >> 4)) * 3 * 64 + ((k >> 3) & 1) * 32 + (row & 31)
            for part in range(3):
                seen.add(((frag + 64 * part) * 8 + (k & 7)))
    assert seen == set(range(4 * 16 * 3 * 64 * 8))


def test_groups_rule():
    """ceil(F / ceil(F / CUs)): the fewest workgroups that keep the frame rounds."""
    def groups(Fr, cus):
        rounds = -(-Fr // cus)
        return -(-Fr // rounds)
    assert groups(640, 256) == 214 and groups(5, 256) == 5 and groups(259, 256) == 130 and groups(256, 256) == 256
    for Fr in range(1, 1200, 7):
        g = groups(Fr, 256)
        assert g <= 256 and -(-Fr // g) == -(-Fr // 256)


# ------------------------------------------------------------ the entry's refusals (no GPU) ----
def _bwd(lib, d, ptrs, mg=0):
    return lib.aaa_vision_enc_f32_bwd(ctypes.byref(d) if d is not None else None, *ptrs[:7], None, mg, ptrs[7], None)


def test_entry_refuses_before_the_device():
    lib = N.load()
    A = 1 << 20
    good = N.EncDesc(2, 84, 84, N.F32, N.FLAG_FRAMES_U8, 192)
    assert lib.aaa_vision_enc_f32_workspace_bytes(ctypes.byref(good)) > 2 * (64 * 512 + 32 * 256 + 32) * 4
    assert lib.aaa_vision_enc_f32_workspace_bytes(ctypes.byref(N.EncDesc(2, 84, 84, N.BF16, 0, 192))) == 0
    assert _bwd(lib, None, [A] * 8) == -1
    assert _bwd(lib, N.EncDesc(2, 84, 84, N.BF16, 0, 192), [A] * 8) == -1
    assert _bwd(lib, good, [A] * 8, mg=-1) == -1
    for i in (0, 1, 2, 3, 4, 6, 7):   # dy1 (5) may be NULL
        ptrs = [A] * 8
        ptrs[i] = None
        assert _bwd(lib, good, ptrs) == -1, i
        ptrs[i] = A + 8
        assert _bwd(lib, good, ptrs) == -2, i   # AAA_E_ALIGN
