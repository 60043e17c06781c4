"""How far the MFMA-bound shapes of cvcl_gemm are from the vendor library: torch.matmul (hipBLASLt / rocBLAS) on the same shapes.
Measurement aid only -- the product never calls the library."""
import os, sys, torch
import timing
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "multimodal-baby_amd"))
from multimodal import _hip as H
dev = torch.device("cuda:0")
shapes = [("l3.conv1", 50176, 512, 1024), ("l3.conv3", 50176, 1024, 512), ("l4.conv1", 12544, 1024, 2048), ("l4.conv3", 12544, 2048, 1024),
          ("l3.0.conv1", 200704, 512, 512), ("l4.0.conv1", 50176, 1024, 1024), ("even.3x512", 49152, 512, 1024), ("even.6x512", 49152, 1024, 512),
          ("vit.qkv", 50432, 2304, 768), ("vit.fc1", 50432, 3072, 768), ("vit.fc2", 50432, 768, 3072), ("4096^3", 4096, 4096, 4096), ("8192^3", 8192, 8192, 8192)]
for name, M, N, K in shapes:
    a = torch.randn(M, K, device=dev).bfloat16(); w = (torch.randn(N, K, device=dev) / K ** 0.5).bfloat16()
    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    wt = w.t()
    t = timing.measure({"ours": lambda: H.gemm(a, w, out=out), "lib": lambda: torch.matmul(a, wt, out=out)})          # the two alternate
    fl = 2.0 * M * N * K
    print(f"{name:12s} M={M:6d} N={N:5d} K={K:5d}: cvcl {timing.text(t['ours'], 1e3):>24s} us {fl/t['ours']['ms']/1e9:6.0f} TF | "
          f"torch.matmul {timing.text(t['lib'], 1e3):>24s} us {fl/t['lib']['ms']/1e9:6.0f} TF")
