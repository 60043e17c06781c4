"""Write tests/golden/alignment.npz from the reference's own alignment arithmetic (CPU, build container only).

    python tools/gen_golden_alignment.py [--reference DIR]

The reference's analysis_tools/representation_similarity.py is loaded as a file (it imports numpy and scipy alone) and its four
helpers run on the seeded inputs of tests/alignment_common.py::golden_inputs (features [157, 64], 7 classes of unequal size with a
singleton, text features [7, 64]).  The torch calls of analysis_cvcl/alignment.py:106-110 (np.mean per category), :142-161 and
:182-195 (one F.normalize / F.cosine_similarity pair per matrix entry), :230-232 (scipy.stats.pearsonr of the upper triangles) and
analysis_cvcl/embeddings.py:106-111 (F.pairwise_distance) are issued here on the same inputs, call for call.  Only these inputs
and outputs are stored.  The float64 restatement the tests use (tests/alignment_common.py) must reproduce the stored fp32 values
to 5e-6 relative, the bound oracle/gen_golden.py holds every other restatement to.  Fixed zip timestamps: re-running reproduces
the archive byte for byte."""
import argparse
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np
import scipy.stats
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "alignment.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import alignment_common as AC                          # noqa: E402


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zf.writestr(info, buf.getvalue())


def maxrel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def torch_sims(a, b):
    """alignment.py:148-161: one normalize / cosine_similarity pair per entry, into a float64 matrix"""
    out = np.zeros((len(a), len(b)))
    for i in range(len(a)):
        for j in range(len(b)):
            x1 = F.normalize(torch.Tensor(a[i]), p=2, dim=0)
            x2 = F.normalize(torch.Tensor(b[j]), p=2, dim=0)
            out[i, j] = F.cosine_similarity(x1, x2, dim=0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("CVCL_REFERENCE", "/root/reference"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_rs", os.path.join(a.reference, "analysis_tools", "representation_similarity.py"))
    rs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rs)

    feats, labels, text = AC.golden_inputs()
    Cn = text.shape[0]
    out = {"features": feats, "labels": labels, "text_features": text}
    # alignment.py:106-110
    means = np.array([np.mean(feats[[j for j in range(len(labels)) if labels[j] == c]], axis=0) for c in range(Cn)])
    out["mean_image_features"] = means
    # alignment.py:142-161, :182-195
    combined = []
    for i in range(Cn):
        combined.append(means[i])
        combined.append(text[i])
    combined = np.array(combined)
    out["combined_sims"] = torch_sims(combined, combined)
    out["image_text_sims"] = torch_sims(means, text)
    out["image_sims"] = torch_sims(means, means)
    out["text_sims"] = torch_sims(text, text)
    # alignment.py:230-232
    iu = out["image_sims"][np.triu_indices_from(out["image_sims"], k=1)]
    tu = out["text_sims"][np.triu_indices_from(out["text_sims"], k=1)]
    res = scipy.stats.pearsonr(iu, tu)
    out["pearson"] = np.array([res[0], res[1], len(iu)], dtype=np.float64)
    # embeddings.py:106-111
    dist = np.zeros(Cn)
    for i in range(Cn):
        dist[i] = F.pairwise_distance(torch.tensor(means[i]).unsqueeze(0), torch.tensor(text[i]).unsqueeze(0), p=2)
    out["paired_distances"] = dist
    # representation_similarity.py, the four helpers
    out["rs_cosine_matrix"] = rs.cosine_matrix(means)
    out["rs_cosine_dissim_matrix"] = rs.cosine_dissim_matrix(means)
    out["rs_strict_upper_tri_items"] = rs.strict_upper_tri_items(out["rs_cosine_matrix"])
    r2 = rs.rsa_of_dissim_matrices(rs.cosine_dissim_matrix(means), rs.cosine_dissim_matrix(text))
    out["rs_rsa"] = np.array([r2[0], r2[1]], dtype=np.float64)

    # the float64 restatement against the reference's fp32 values
    m64 = AC.class_means64(feats, labels, Cn)
    errs = {
        "mean_image_features": maxrel(m64, means),
        "image_sims": maxrel(AC.cosine64(means), out["image_sims"]),
        "text_sims": maxrel(AC.cosine64(text), out["text_sims"]),
        "image_text_sims": maxrel(AC.cosine64(means, text), out["image_text_sims"]),
        "combined_sims": maxrel(AC.cosine64(AC.interleave(means, text)), out["combined_sims"]),
        "rs_cosine_matrix": maxrel(AC.cosine64(means), out["rs_cosine_matrix"]),
        "rs_cosine_dissim_matrix": maxrel(AC.dissim64(means), out["rs_cosine_dissim_matrix"]),
        "rs_strict_upper_tri_items": maxrel(AC.triu_items(AC.cosine64(means)), out["rs_strict_upper_tri_items"]),
        "pearson_r": abs(AC.rsa64(AC.cosine64(means), AC.cosine64(text)) - res[0]) / abs(res[0]),
        "rs_rsa_r": abs(AC.rsa64(AC.dissim64(means), AC.dissim64(text)) - r2[0]) / abs(r2[0]),
        "paired_distances": maxrel(AC.paired_l2_64(means, text), dist),
    }
    for k, v in errs.items():
        print(f"alignment {k}: restatement-vs-reference rel err {v:.2e}")
        assert v <= 5e-6, (k, v)
    # the Pearson condition of the GPU tests: the triangles of these inputs spread, and the reference's own fp32 loop is inside the bound
    bound, sigma = AC.pearson_bound(feats.shape[1], AC.triu_items(AC.cosine64(m64)), AC.triu_items(AC.cosine64(text)))
    r64 = AC.rsa64(AC.cosine64(m64), AC.cosine64(text))
    print(f"alignment pearson: sigma_min {sigma:.4f}, bound {bound:.3e}, reference fp32 loop error {abs(res[0] - r64):.3e}")
    assert sigma >= 0.05 and abs(res[0] - r64) <= bound
    write_npz(OUT, out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
