"""Write tests/golden/ngram.npz from the reference's own n-gram model (its top-level ngram.py; CPU, build container only).

    python tools/gen_golden_ngram.py [--reference DIR]

For every case (N, vocab_size, B, L) of tests/ngram_common.py CASES: the reference's NGramModel is updated with the training
corpus (seed N) and scores the evaluation corpus (seed 100 + N) at alpha 0.1 and 0.4.  Recorded per case: both corpora, the
reference's counts (per order the context tuples, words, counts and context totals, in sorted order), its float32 token losses
and its ``tokenwise=False`` scalar per alpha.  Data only; fixed zip timestamps: re-running reproduces the archive byte for byte."""
import argparse
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "ngram.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))


def load_reference(ref_dir):
    spec = importlib.util.spec_from_file_location("ref_ngram", os.path.join(ref_dir, "ngram.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zf.writestr(info, buf.getvalue())


def main():
    import ngram_common as NC
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("CVCL_REFERENCE", "/root/reference"))
    a = ap.parse_args()
    ref = load_reference(a.reference)
    out = {"cases": np.array(NC.CASES, dtype=np.int64), "alphas": np.array(NC.ALPHAS, dtype=np.float64)}
    for case in NC.CASES:
        N, V, B, L = case
        name = NC.case_name(case)
        (ty, tl), (ey, el) = NC.case_data(case)
        out.update({f"{name}.train_y": ty, f"{name}.train_len": tl, f"{name}.eval_y": ey, f"{name}.eval_len": el})
        model = ref.NGramModel(N, V)
        model.update(torch.from_numpy(ty), torch.from_numpy(tl))
        for n, table in enumerate(model._count):
            rows = sorted((ctx, w, c, total) for ctx, (total, nxt) in table.items() for w, c in nxt.items())
            out[f"{name}.count{n}.ctx"] = np.array([r[0] for r in rows], dtype=np.int64).reshape(len(rows), n)
            out[f"{name}.count{n}.word"] = np.array([r[1] for r in rows], dtype=np.int64)
            out[f"{name}.count{n}.cnt"] = np.array([r[2] for r in rows], dtype=np.int64)
            out[f"{name}.count{n}.total"] = np.array([r[3] for r in rows], dtype=np.int64)
        for alpha in NC.ALPHAS:
            loss = model.calculate_ce_loss(torch.from_numpy(ey), torch.from_numpy(el), alpha=alpha)
            mean = model.calculate_ce_loss(torch.from_numpy(ey), torch.from_numpy(el), alpha=alpha, tokenwise=False)
            assert loss.dtype == torch.float32 and tuple(loss.shape) == (B, L - 1)
            out[f"{name}.loss_a{alpha}"] = loss.numpy()
            out[f"{name}.mean_a{alpha}"] = np.array(mean.item(), dtype=np.float32)
    write_npz(OUT, out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
