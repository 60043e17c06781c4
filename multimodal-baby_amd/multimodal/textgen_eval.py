"""Caption scores for eval_textgen (reference multimodal/textgen_eval.py): BLEU-1..4, ROUGE-L and CIDEr as pycocoevalcap defines
them with default arguments and no PTB tokenizer, computed on the device (ops.caption_scores, csrc/textgen_scores.hip).  The
package's own BLEU, ROUGE and CIDEr are not called.  METEOR, which needs a Java runtime, is added only when pycocoevalcap imports;
SPICE is not computed.

Tokens are ``sentence.split()``.  The package's ROUGE splits on ``" "`` instead: the two differ only on repeated or leading spaces
and on the empty string, where both score 0."""
from __future__ import annotations

import torch

from . import ops


def _meteor(refs, hyps):
    try:
        from pycocoevalcap.meteor.meteor import Meteor
    except Exception:                                        # not installed (it is not a dependency of this package)
        return {}
    score, _ = Meteor().compute_score({i: r for i, r in enumerate(refs)}, {i: [h] for i, h in enumerate(hyps)})
    return {"METEOR": score}


def _rows(sentences, device):
    """token-id lists -> (ids [len(sentences), widest or 1] int64, zero padded, lengths) on ``device``"""
    width = max(1, max(map(len, sentences)))
    ids = torch.tensor([s + [0] * (width - len(s)) for s in sentences], dtype=torch.int64)
    return ids.to(device), torch.tensor([len(s) for s in sentences], dtype=torch.int64).to(device)


def evaluate(list_of_references, hypotheses, keys=None):
    """list_of_references[i]: the reference sentence(s) of example i (a string or a list of strings); hypotheses[i]: the
    generated sentence; ``keys`` is accepted as the reference accepts it and not used.  -> {"BLEU_1", .., "BLEU_4", "ROUGE_L",
    "CIDEr": float} (and "METEOR" when pycocoevalcap imports).  The words of references and hypotheses are interned into ids in
    one pass on the host; a corpus over a limit of include/cvcl_hip.h "Caption scores" (128 tokens per sentence, 32 references per
    example, 32768 distinct words) raises CvclError naming it.  There is no CPU path."""
    if len(list_of_references) != len(hypotheses) or not len(hypotheses):
        raise ValueError(f"evaluate: {len(list_of_references)} reference entries for {len(hypotheses)} hypotheses (at least one of each)")
    refs = [list(r) if isinstance(r, (list, tuple)) else [r] for r in list_of_references]
    ids = {}
    intern = lambda sentence: [ids.setdefault(w, len(ids)) for w in sentence.split()]          # noqa: E731
    hyp = [intern(h) for h in hypotheses]
    ref = [intern(s) for r in refs for s in r]
    offsets = [0]
    for r in refs:
        offsets.append(offsets[-1] + len(r))
    device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")        # (ops refuses CPU tensors)
    scores, _ = ops.caption_scores(*_rows(hyp, device), *_rows(ref or [[]], device), torch.tensor(offsets).to(device), max(1, len(ids)))
    scores.update(_meteor(refs, hypotheses))
    return scores
