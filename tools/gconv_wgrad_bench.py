"""cvcl_gconv3x3_wgrad on the trunk's shapes at B = 256 (bf16): time per call."""
import os, sys, torch
import timing
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "multimodal-baby_amd"))
from multimodal import _hip as H
dev = torch.device("cuda:0"); lib = H.lib(); B = 256
for C, S, stride in ((128, 56, 1), (256, 56, 2), (256, 28, 1), (512, 28, 2), (512, 14, 1), (1024, 14, 2), (1024, 7, 1)):
    So = (S - 1) // stride + 1
    x = torch.randn(B, S, S, C, device=dev).bfloat16(); dy = torch.randn(B, So, So, C, device=dev).bfloat16()
    dw = torch.empty(C, C // 32, 3, 3, device=dev)
    nb = lib.cvcl_gconv3x3_wgrad_workspace_bytes(B, S, S, C, stride)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    def run():
        H.check(lib.cvcl_gconv3x3_wgrad(H.ptr(x), H.ptr(dy), H.ptr(dw), B, S, S, C, 32, stride, H.ptr(ws), nb, H.stream_ptr()), "wgrad")
    t = timing.measure({"run": run})["run"]
    mb = (x.numel() + dy.numel()) * 2 / 1e6
    print(f"C {C:5d} {S:3d}x{S:<3d} stride {stride}: {timing.text(t, 1e3):>24s} us  (x + dy = {mb:6.1f} MB, one pass at 5.5 TB/s = {mb / 5.5:5.1f} us)")
