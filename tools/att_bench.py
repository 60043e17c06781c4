"""Timing of cvcl_attention alone at the C4 shapes (B = 256, 12 heads x 64; 197 and 257 tokens); CVCL_HIP_LIB selects the library."""
import os, sys, torch
import timing
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "multimodal-baby_amd"))
from multimodal import _hip as H
dev = torch.device("cuda:0")
for T in (197, 257):
    B, heads, D = 256, 12, 768
    qkv = torch.randn(B * T, 3 * D, device=dev).bfloat16()
    out = torch.empty(B * T, D, dtype=torch.bfloat16, device=dev)
    def call():
        H.check(H.lib().cvcl_attention(H.BF16, H.ptr(qkv), None, H.ptr(out), B, T, heads, 64, 0.125, H.stream_ptr()), "cvcl_attention")
    print(os.path.basename(os.environ.get("CVCL_HIP_LIB", "(product)")), f"T={T}: {timing.text(timing.measure({'call': call})['call'], 1e3)} us")
