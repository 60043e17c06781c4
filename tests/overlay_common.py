"""What the attention-overlay tests share: the case table, the seeded inputs, the float64 restatement of getAttMap's arithmetic
(F.interpolate bicubic on float64, scipy.ndimage.gaussian_filter on float64, numpy for the rest) and the bounds.

Bounds (DESIGN.md "Attention overlays"):
  MAP_BOUND  |x - x_ref| <= 1e-5 on the normalised map: two filter passes of at most 37 fp32 products each with weights summing to 1
             give about 2 * 38 * 2^-24 * max|m| = 4.5e-6 relative to the range where range >= max|m| (every case but the blurred 8 x 200
             one, whose range is a third of its maximum: 1.3e-5 in the worst case, a few 1e-7 for random rounding errors).
  out_f32    off the colour-table edges |out - ref| <= MAP_BOUND ** 0.7 + MAP_BOUND (x ** 0.7 is Hoelder-0.7 with constant 1; the frame
             and the colour are within [0, 1]); on a near-edge pixel the table's largest
             adjacent-entry step is added.  A pixel is near an edge when x_ref * n_lut lies within n_lut * MAP_BOUND of one of the
             integers 1 .. n_lut - 1 (0 and n_lut are the ends of the table, not edges: x within MAP_BOUND of them keeps its entry).
  share      the near-edge pixels are at most max(2 %, 4 * n_lut * MAP_BOUND) of a case: twice what a uniform density of x gives.
  out_u8     at most 1 count from floor(clamp(ref) * 255 + 0.5) off the edges, 1 + ceil(255 * step) on them."""
import math

import numpy as np
import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
MAP_BOUND = 1e-5
F32_BOUND = MAP_BOUND ** 0.7 + MAP_BOUND
GAMMA = 0.7

# name -> (N, M, (h, w), (H, W), image_of_map or None)
CASES = {
    "workload_7x7_224": (2, 2, (7, 7), (224, 224), None),                    # the workload's own geometry, radius 18
    "vit_16x16_64x96": (1, 3, (16, 16), (64, 96), [0, 0, 0]),                # non-square, radius 8, ViT-style grid
    "odd_3x3_37x53": (2, 5, (3, 3), (37, 53), [0, 0, 1, 1, 1]),              # off every tile boundary, shared images, radius 4
    "noresize_8x200": (1, 1, (8, 200), (8, 200), None),                      # radius 16 exceeds H: repeated reflection
    # degenerate output sizes (radius 0; one pixel is a constant map).  The entry's limits are 1 <= h <= H, 1 <= w <= W, so the maps
    # are the largest those allow rather than 5 x 5
    "degenerate_1x1": (1, 2, (1, 1), (1, 1), [0, 0]),
    "degenerate_2x3": (1, 2, (2, 3), (2, 3), [0, 0]),
}


def make_maps(M, h, w, seed):
    """rand(h, w).clamp(min=0.3) - 0.3 per seed"""
    return torch.stack([torch.rand(h, w, generator=torch.Generator().manual_seed(seed + m)).clamp(min=0.3) - 0.3 for m in range(M)])


def make_images(N, H, W, seed, overshoot=0.0):
    """normalised frames whose de-normalised values cover [-overshoot, 1 + overshoot] (0: what the out_f32 bound assumes; 0.1 in the
    exact tests: both clamps of the uint8 conversion are exercised)"""
    g = torch.Generator().manual_seed(1000 + seed)
    frame = torch.rand(N, 3, H, W, generator=g) * (1.0 + 2.0 * overshoot) - overshoot
    return ((frame - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)).contiguous()


def viridis():
    import matplotlib
    cm = matplotlib.colormaps["viridis"]
    return np.ascontiguousarray(cm(np.arange(cm.N))[:, :3], dtype=np.float64)      # (the device gets its fp32 rounding)


def lut_step(lut):
    """the largest adjacent-entry step of a colour table"""
    return float(np.abs(np.diff(np.asarray(lut, dtype=np.float64), axis=0)).max())


def frames64(images, mean=MEAN, std=STD):
    """[N, H, W, 3] float64: img * std + mean"""
    x = images.double().numpy()
    return (x * np.asarray(std).reshape(1, 3, 1, 1) + np.asarray(mean).reshape(1, 3, 1, 1)).transpose(0, 2, 3, 1)


def blurred64(maps, size, blur):
    """[M, H, W] float64: the maps at the output size, blurred as getAttMap blurs them"""
    from scipy.ndimage import gaussian_filter
    m = maps.double()
    if tuple(m.shape[-2:]) != tuple(size):
        m = F.interpolate(m[:, None], size=tuple(size), mode="bicubic", align_corners=False)[:, 0]
    m = m.numpy()
    if blur:
        m = np.stack([gaussian_filter(a, 0.02 * max(size)) for a in m])
    return m


def reference(maps, images, image_of_map, lut, blur=True, vmin=None, vmax=None, gamma=GAMMA):
    """-> dict: x [M, H, W], out [M, H, W, 3] float64, u8 [M, H, W, 3], near [M, H, W] bool (near-edge pixels), lo / hi per map"""
    size = tuple(images.shape[2:])
    m = blurred64(maps, size, blur)
    fr = frames64(images)
    lut64 = np.asarray(lut, dtype=np.float64)
    n = lut64.shape[0]
    xs, outs, los, his = [], [], [], []
    for i, a in enumerate(m):
        lo, hi = (a.min(), a.max()) if vmin is None else (float(vmin), float(vmax))
        x = (a - lo) / (hi - lo) if hi > lo else a - lo
        if vmin is not None:
            x = np.clip(x, 0.0, 1.0)                                         # the one documented deviation from getAttMap
        idx = np.minimum((x * n).astype(np.int64), n - 1)
        wgt = (x ** gamma)[..., None]
        img = fr[i if image_of_map is None else image_of_map[i]]
        outs.append((1 - wgt) * img + wgt * lut64[idx])
        xs.append(x)
        los.append(lo)
        his.append(hi)
    x, out = np.stack(xs), np.stack(outs)
    t = x * n
    k = np.clip(np.rint(t), 1, n - 1)
    near = np.abs(t - k) <= n * MAP_BOUND
    return {"x": x, "out": out, "u8": np.floor(np.clip(out, 0, 1) * 255 + 0.5).astype(np.int64), "near": near, "lo": los, "hi": his,
            "blurred": m}


def share_limit(n_lut):
    return max(0.02, 4 * n_lut * MAP_BOUND)


def check_against_reference(ref, lut, out_map=None, out_f32=None, out_u8=None, label=""):
    """the assertions of the module docstring; prints every figure before it asserts"""
    step = lut_step(lut)
    near = ref["near"]
    share = float(near.mean())
    print(f"{label}: near-edge share {share:.4%} (limit {share_limit(len(lut)):.2%}), table step {step:.4f}")
    assert share <= share_limit(len(lut)), (label, share)
    if out_map is not None:
        e = float(np.abs(out_map.astype(np.float64) - ref["x"]).max())
        print(f"{label}: out_map max error {e:.3e} (bound {MAP_BOUND:.0e})")
        assert e <= MAP_BOUND, (label, e)
    if out_f32 is not None:
        d = np.abs(out_f32.astype(np.float64) - ref["out"]).max(-1)
        off, on = float(d[~near].max()) if (~near).any() else 0.0, float(d[near].max()) if near.any() else 0.0
        print(f"{label}: out_f32 max error off the edges {off:.3e} (bound {F32_BOUND:.3e}), on them {on:.3e} (bound {F32_BOUND + step:.3e})")
        assert np.isfinite(out_f32).all() and off <= F32_BOUND and on <= F32_BOUND + step, (label, off, on)
    if out_u8 is not None:
        d = np.abs(out_u8.astype(np.int64) - ref["u8"]).max(-1)
        off, on = int(d[~near].max()) if (~near).any() else 0, int(d[near].max()) if near.any() else 0
        print(f"{label}: out_u8 max error off the edges {off} (bound 1), on them {on} (bound {1 + math.ceil(255 * step)})")
        assert off <= 1 and on <= 1 + math.ceil(255 * step), (label, off, on)
