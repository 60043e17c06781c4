"""Caption scores for eval_textgen (reference multimodal/textgen_eval.py): BLEU-1..4, METEOR, ROUGE-L, CIDEr through
pycocoevalcap when that package imports.  It is optional: without it a warning is printed once and no scores are logged."""
from __future__ import annotations

import warnings

_warned = False


def _scorers():
    global _warned
    try:
        from pycocoevalcap.bleu.bleu import Bleu
        from pycocoevalcap.cider.cider import Cider
        from pycocoevalcap.meteor.meteor import Meteor
        from pycocoevalcap.rouge.rouge import Rouge
    except Exception as e:                                   # not installed (it is not a dependency of this package)
        if not _warned:
            warnings.warn(f"pycocoevalcap is not available ({e}); text-generation scores are not computed")
            _warned = True
        return None
    return [(Bleu(4), ["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4"]), (Meteor(), "METEOR"), (Rouge(), "ROUGE_L"), (Cider(), "CIDEr")]


def evaluate(list_of_references, hypotheses):
    """list_of_references[i]: the reference sentence(s) of example i (a string or a list of strings); hypotheses[i]: the
    generated sentence.  -> {metric: score}, empty without pycocoevalcap."""
    scorers = _scorers()
    if scorers is None:
        return {}
    refs = {i: list(r) if isinstance(r, (list, tuple)) else [r] for i, r in enumerate(list_of_references)}
    hyps = {i: [h] for i, h in enumerate(hypotheses)}
    out = {}
    for scorer, names in scorers:
        score, _ = scorer.compute_score(refs, hyps)
        if isinstance(names, list):
            out.update(dict(zip(names, score)))
        else:
            out[names] = score
    return out
