"""Shared by the tests of the rollout's discard variant (csrc/vit_discard.hip): the definition restated on the CPU, and the chain /
head fusion / row-relative error of tests/test_vit_rollout_gpu.py.

discard_ref: per [T, T] matrix, flattened row-major to M = T T elements, S = the first k indices of a STABLE ascending sort (ties go
to the lowest flat index); every element with its index in S \\ {0} becomes +0.0, every other element keeps its bits; flat index 0 is
never zeroed but counts towards k."""
import torch


def discard_ref(F, k):
    """F [..., T, T] (any float dtype, CPU) -> a new tensor with the k weakest elements of every matrix zeroed."""
    T = F.shape[-1]
    assert F.shape[-2] == T and 0 <= k <= T * T - 1
    flat = F.reshape(-1, T * T).clone()
    order = torch.sort(flat, dim=-1, stable=True).indices[:, :k]
    mask = torch.zeros_like(flat, dtype=torch.bool)
    mask.scatter_(1, order, True)
    mask[:, 0] = False
    flat[mask] = 0.0
    return flat.reshape(F.shape)


def fuse(P, fusion):
    """[B, heads, T, T] -> [B, T, T]."""
    return P.mean(1) if fusion == "mean" else (P.max(1).values if fusion == "max" else P.min(1).values)


def chain(Fs, start_layer=0, q_rows=None):
    """Fs: the fused matrices [B, T, T] in block order, any dtype -> the first q_rows rows of A^_last ... A^_start_layer."""
    eye = torch.eye(Fs[0].shape[-1], dtype=Fs[0].dtype)
    R = None
    for Fl in Fs[start_layer:]:
        A = Fl + eye
        A = A / A.sum(-1, keepdim=True)
        R = A if R is None else A @ R
    return R if q_rows is None else R[:, :q_rows]


def row_rel(got, ref64):
    """Worst |got - ref| over the largest element of the row of ref."""
    return float(((got.double() - ref64).abs() / ref64.abs().amax(-1, keepdim=True)).max())
