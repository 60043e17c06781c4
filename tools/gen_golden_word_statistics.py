"""Generate tests/golden/word_statistics.npz from the reference's own word-level analysis, run on the CPU.

    python tools/gen_golden_word_statistics.py [REFERENCE_CHECKOUT]

The reference's get_model_items, get_token_items and get_model_probs (analysis_tools/processing.py) and its SumData
(analysis_tools/sumdata.py) are driven on a stub model: the reference's real TextEncoder + LanguageModel at toy size (V = 50,
E = H = 32; formula-filled as tools/gen_golden_captioning.py fills them, output bias ce_bias) behind the three members
processing.py touches of a MultiModalLitModel (``language_model``, ``text_encoder``, ``calculate_ce_loss(y, y_len, x=...)``).  Two
models: ``plain``, a regressional LSTM LM, and ``captioning``, whose LSTM starts from the connector's state of the batch's ``x``
(flat image features stand in for the images: the stub's image encoder is the identity).

Data: 12 utterances of 2 to 9 tokens in two batches padded to 9 and to 6, words from a pool of 12 so that keys repeat, tags from
{NN, VB, DT} by a formula of word and position (``.`` for <sos> / <eos>), arranged so that word 30 occurs once as NN and once as VB
(the count tie of get_token_items), word 40 occurs once, and utterance 3 has two tags fewer than tokens.

The file holds data only: the inputs and, per model, what the reference returned (losses, the two item tables as arrays in
sorted key order, the probabilities per tagged position).  The tests rebuild the weights from the formula.  Fixed zip timestamps:
re-running reproduces the archive byte for byte.
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden  # noqa: E402
import gen_golden_captioning as GC  # noqa: E402

V, E = 50, 32
LENGTHS = ((9, 5, 2, 7, 4, 9, 3), (6, 4, 2, 5, 3))
PAD_LEN = (9, 6)
WORD_TAGS = ("NN", "VB", "DT")
TOP_K = 5
SEED = 1                                                    # of the words and image features; see EXACT_K
# The toy LMs' distributions are flat (largest probability of a position ~0.1, sixth best >= 0.03), so neighbouring probabilities
# come close: the smallest gaps among the six best of a position are, by rank, 4.5e-4, 3.6e-4, 5.3e-5, 2.4e-4, 1.2e-4 (plain) and
# 8.6e-4, 4.0e-4, 1.4e-4, 2.1e-4, 5.6e-5 (captioning).  The best EXACT_K + 1 of every position lie > 1e-4 apart (asserted below);
# no seed among 1 .. 150 separates all six by 1.5e-4.
EXACT_K = 2


class StubLit(nn.Module):
    """What analysis_tools/processing.py touches of a MultiModalLitModel."""

    def __init__(self, language_model):
        super().__init__()
        self.language_model = language_model
        self.text_encoder = language_model.text_encoder

    def calculate_ce_loss(self, y, y_len, x=None, image_features=None, image_feature_map=None, **kwargs):
        if self.text_encoder.captioning and image_features is None:
            image_features = x                              # the image encoder of the stub: the identity on flat features
        if not self.text_encoder.captioning:
            image_features = None
        return self.language_model.calculate_ce_loss(y, y_len, image_features=image_features, **kwargs)


def data(seed=SEED):
    """-> (batches [(x, y, y_len, raw_y)], pos_tags)"""
    g = torch.Generator().manual_seed(seed)
    batches, pos_tags = [], []
    for lens, pad in zip(LENGTHS, PAD_LEN):
        B = len(lens)
        y = torch.zeros(B, pad, dtype=torch.long)
        for b, n in enumerate(lens):
            y[b, 0] = 2
            y[b, 1:n - 1] = torch.randint(4, 16, (n - 2,), generator=g)
            y[b, n - 1] = 3
        x = torch.randn(B, E, generator=g) * 0.5
        batches.append([x, y, torch.tensor(lens), None])
    y0, y1 = batches[0][1], batches[1][1]
    y0[0, 4], y1[0, 2] = 30, 30                             # word 30: once NN, once VB (tags below)
    y0[5, 6] = 40                                           # word 40: once
    for bi, (x, y, y_len, _r) in enumerate(batches):
        raw = []
        for b in range(len(y)):
            n = int(y_len[b])
            toks = y[b, :n].tolist()
            tags = ["." if t in (2, 3) else WORD_TAGS[(t * 7 + l) % 3] for l, t in enumerate(toks)]
            for l, t in enumerate(toks):
                if t == 30:
                    tags[l] = "NN" if bi == 0 else "VB"
            pos_tags.append(tags)
            raw.append([" ".join(f"w{t}" for t in toks[1:-1])])
        batches[bi] = (x, y, y_len, raw)
    pos_tags[3] = pos_tags[3][:-2]                          # a tag list shorter than its utterance
    return batches, pos_tags


def import_reference_processing():
    """The reference's analysis_tools.processing; modules it imports at the top but that the calls made here never reach are
    stubbed when they are not installed."""
    import types

    class Anything:
        """Stands for any name of a stubbed module: callable, and every attribute is again Anything."""

        def __call__(self, *a, **k):
            return a[0] if a else Anything()                # tqdm(iterable) -> iterable

        def __getattr__(self, name):
            return Anything()

    class Stub(types.ModuleType):
        __path__ = []

        def __getattr__(self, name):
            return Anything()

    roots = ("tqdm", "huggingface_hub", "PIL")
    missing = {root for root in roots if root not in sys.modules and importlib.util.find_spec(root) is None}
    for name in roots:
        if name.split(".")[0] in missing:
            sys.modules[name] = Stub(name)
    # analysis_tools/word_ratings.py reads a spreadsheet from its authors' file system at import; nothing of it is used here
    sys.modules["analysis_tools.word_ratings"] = types.ModuleType("analysis_tools.word_ratings")
    from analysis_tools import processing
    return processing


def items_arrays(series):
    """A Series of SumData indexed by (token_id, pos), sorted -> arrays in that order."""
    keys = list(series.index)
    vals = list(series.values)
    return {"token_id": np.array([k[0] for k in keys], dtype=np.int64), "pos": np.array([k[1] for k in keys]),
            "cnt": np.array([int(v.cnt) for v in vals], dtype=np.int64), "loss": np.array([float(v.loss) for v in vals], dtype=np.float64),
            "vector": np.stack([np.asarray(v.vector, dtype=np.float32) for v in vals])}


def main():
    if len(sys.argv) > 1:
        gen_golden.REF = sys.argv[1]
    gen_golden.install_stubs()
    from multimodal import multimodal as mm
    P = import_reference_processing()
    torch.set_num_threads(4)
    batches, pos_tags = data(SEED)
    out = {"cases": np.array(["plain", "captioning"]), "pos_tags": np.array([" ".join(t) for t in pos_tags]), "top_k": np.array([TOP_K]),
           "exact_k": np.array([EXACT_K])}
    for i, (x, y, y_len, _raw) in enumerate(batches):
        out[f"x{i}"], out[f"y{i}"], out[f"y_len{i}"] = x.numpy(), y.numpy(), y_len.numpy()
    n_tagged = sum(min(len(t), int(n)) for t, n in zip(pos_tags, [n for lens in LENGTHS for n in lens]))
    for name, captioning in (("plain", False), ("captioning", True)):
        te, lm = GC.build(mm, captioning, V=V, E=E)
        with torch.no_grad():
            lm.output_layer.bias.copy_(GC.ce_bias(V))
        model = StubLit(lm).eval()
        items = P.get_model_items(model, batches, pos_tags)
        assert items.all_token_items is None
        losses = np.zeros((len(pos_tags), max(PAD_LEN)), dtype=np.float32)
        for r, l in enumerate(items.losses):
            losses[r, :len(l)] = l
        out[f"{name}.losses"] = losses
        for table, series in (("token_pos_items", items.token_pos_items), ("token_items", items.token_items)):
            for k, a in items_arrays(series).items():
                out[f"{name}.{table}.{k}"] = a
        emb = np.stack([np.asarray(v.embedding) for v in items.token_items.values])
        assert np.array_equal(emb, te.embedding.weight.detach().numpy()[out[f"{name}.token_items.token_id"]])
        probs = P.get_model_probs(model, batches, pos_tags)
        out[f"{name}.probs.token_id"] = np.array([k[0] for k in probs.index], dtype=np.int64)
        out[f"{name}.probs.pos"] = np.array([k[1] for k in probs.index])
        out[f"{name}.probs"] = np.stack(list(probs.values)).astype(np.float32)
        assert len(probs) == n_tagged == int(out[f"{name}.token_pos_items.cnt"].sum())
        p64 = np.sort(out[f"{name}.probs"].astype(np.float64), axis=1)[:, ::-1][:, :EXACT_K + 1]
        live = p64[:, 0] > 0
        gap = float((p64[live, :-1] - p64[live, 1:]).min())
        assert gap > 1e-4, gap
        tpi, ti = out[f"{name}.token_pos_items.cnt"], out[f"{name}.token_items.cnt"]
        print(f"{name}: {len(tpi)} (word, tag) keys, {len(ti)} words, {n_tagged} tagged positions, largest segment {int(tpi.max())}, "
              f"max loss {losses.max():.3f}; smallest gap among the top {EXACT_K + 1} probabilities of a position {gap:.2e}")
    path = os.path.join(ROOT, "tests", "golden", "word_statistics.npz")
    GC.write_npz(path, out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
