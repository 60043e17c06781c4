"""Timing of the grouped-conv kernel on the trunk's shapes; CVCL_HIP_LIB selects the library."""
import os, sys, torch
import timing
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "multimodal-baby_amd"))
from multimodal import _hip as H
dev = torch.device("cuda:0")
def run(B, S, C, stride):
    cg = C // 32
    x = torch.randn(B, S, S, C, device=dev).to(torch.bfloat16)
    w = torch.randn(C, cg, 3, 3, device=dev)
    nb = H.lib().cvcl_packed_weight_bytes(H.BF16, H.PACK_GCONV3, C, cg, 3)
    wp = torch.empty(nb, dtype=torch.uint8, device=dev)
    H.check(H.lib().cvcl_pack_conv_weight(H.BF16, H.PACK_GCONV3, H.ptr(w), H.ptr(wp), C, cg, 3, H.stream_ptr()), "pack")
    sc, sh = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    So = (S - 1) // stride + 1
    y = torch.empty(B, So, So, C, dtype=torch.bfloat16, device=dev)
    rows = H.lib().cvcl_gconv3x3_stats_rows(H.BF16, B, S, S, C, stride)
    st = torch.empty(rows, 2, C, device=dev)
    def call():
        H.check(H.lib().cvcl_gconv3x3(H.BF16, H.ptr(x), H.ptr(sc), H.ptr(sh), H.ptr(wp), H.ptr(y), H.ptr(st), rows, None, B, S, S, C, 32, stride, H.stream_ptr()), "gconv")
    return timing.text(timing.measure({"call": call})["call"], 1e3, ".0f")
print("lib%s  layer1(56,128,s1): %s us   layer2.0(56,256,s2): %s us   layer2(28,256,s1): %s us   layer3(14,512): %s us" % (
    os.path.basename(os.environ.get("CVCL_HIP_LIB", "")), run(256, 56, 128, 1), run(256, 56, 256, 2), run(256, 28, 256, 1), run(256, 14, 512, 1)))
