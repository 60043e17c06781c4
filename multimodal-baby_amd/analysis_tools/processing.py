"""Word-level language-model analysis on the HIP path (the interface of the reference's analysis_tools/processing.py:
run_model .. get_model_probs).

The reference visits every token in Python -- an ``.item()``, a ``SumData.__add__`` and, for the predictions, a host softmax over
the vocabulary per position.  Here a batch is one LM forward (HIP already), one host CSR build over the (word, tag) keys present
in it (the tags are host strings) and one cvcl_token_items_accumulate launch; the key tables stay on the device until the end.
The predictions are one cvcl_token_topk launch per batch.  Items are plain dicts in sorted key order; ``build_series`` turns
them into the reference's pandas Series.

The baseline the reference sets beside the language model, its back-off n-gram model, runs through the same functions: an
``ngram.NGramModel`` (``build_ngram_model``) is regressional, has ``outputs`` of width 0, takes its token losses from one
cvcl_ngram_ce_loss launch per batch and its predictions from cvcl_ngram_probs (the back-off score of every word; the reference
has no predictions for an n-gram).  The smoothing weight is the model's ``alpha`` attribute.

Attention language models and ``model is None`` are outside the implemented path (NotImplementedError), and so is an object
that only carries the name NGramModel; there is no CPU fallback."""
import itertools
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import ngram
from multimodal import _hip as H
from multimodal import ops
from multimodal.multimodal_data_module import PAD_TOKEN_ID
from multimodal.utils import map_structure

from .sumdata import SumData, zero_sum_data, zero_sum_data_like  # noqa: F401
from .token_items_data import Key
from .utils import get_model_device

ModelItems = namedtuple("ModelItems", ["losses", "all_token_items", "token_pos_items", "token_items"])


def _language_model_of(model):
    """The LM of a model this path runs, or NotImplementedError (no model, n-gram models, attention LMs)."""
    if model is None:
        raise NotImplementedError("model is None (the reference's zero baseline) is outside the implemented path")
    lm = getattr(model, "language_model", None)
    if lm is None or type(model).__name__ == "NGramModel":
        raise NotImplementedError(f"{type(model).__name__}: n-gram models are outside the implemented path "
                                  "(a model with a language_model is needed)")
    if lm.text_encoder.has_attention:
        raise NotImplementedError("attention language models are outside the implemented path")
    return lm


def is_regressional(model):
    """Whether the model predicts token l + 1 at position l, so that its loss, logits and labels are shifted by one."""
    return model is not None and (isinstance(model, ngram.NGramModel) or _language_model_of(model).text_encoder.regressional)


def build_ngram_model(N, vocab_size, train_dataloader, device=None):
    """The n-gram baseline counted over a training set (reference :17-23): one ``update`` per batch."""
    ngram_model = ngram.NGramModel(N, vocab_size, device=device)
    for batch in train_dataloader:
        ngram_model.update(*_tokens_of(batch))
    return ngram_model


def _run_ngram(model, y, y_len, single_example, return_all):
    """run_model for an n-gram model (reference :165-196): no hidden vectors, the loss of calculate_ce_loss; with ``return_all``
    logits = log(calculate_probs), no attention maps, labels = y[:, 1:]."""
    if single_example:
        y, y_len = y.unsqueeze(0), y_len.unsqueeze(0)
    loss = F.pad(model.calculate_ce_loss(y, y_len, alpha=model.alpha, tokenwise=True), (1, 0))
    ret = (torch.zeros(*y.shape, 0, dtype=torch.float32, device=model.device), loss)
    if return_all:
        ret = ret + (model.calculate_probs(y, y_len, alpha=model.alpha).log(), None, y[:, 1:].to(device=model.device, dtype=torch.int64))
    if single_example:
        ret = map_structure(lambda t: t.squeeze(0) if t is not None else None, ret)
    return ret


def examples_from_batches(batches):
    return itertools.chain.from_iterable(zip(*batch) for batch in batches)


def run_model(model, y, y_len, x=None, image_features=None, image_feature_map=None, single_example=False, return_all=False):
    """-> (outputs [B, L, H], loss [B, L]) and, with ``return_all``, (logits, attns, labels) (reference :158-205).  The loss of
    a regressional model is padded with a leading 0 so that column l belongs to token l.  An n-gram model has H = 0 and takes
    only ``y`` and ``y_len``."""
    if isinstance(model, ngram.NGramModel):
        return _run_ngram(model, y, y_len, single_example, return_all)
    lm = _language_model_of(model)
    if image_feature_map is not None:
        raise NotImplementedError("attention language models are outside the implemented path")
    device = get_model_device(model)
    if device.type != "cuda":
        raise H.CvclError("the word statistics run on the HIP path: the model is on the CPU and there is no CPU fallback")
    batch = (x, y, y_len) if x is not None else (y, y_len)
    if single_example:
        batch = map_structure(lambda t: t.unsqueeze(0), batch)
    batch = map_structure(lambda t: t.to(device=device), batch)
    (x, y, y_len) = batch if x is not None else (None,) + tuple(batch)
    loss, outputs, logits, attns, labels = model.calculate_ce_loss(y, y_len, x=x, image_features=image_features, tokenwise=True)
    if lm.text_encoder.regressional:
        loss = F.pad(loss, (1, 0))
    ret = (outputs, loss)
    if return_all:
        ret = ret + (logits, attns, labels)
    if single_example:
        ret = map_structure(lambda t: t.squeeze(0) if t is not None else None, ret)
    return ret


def _tokens_of(batch):
    """(y, y_len) of a batch in either form run_model_on_batches accepts."""
    if isinstance(batch, dict):
        return batch["y"], batch["y_len"]
    return batch[1], batch[2]


def run_model_on_batches(model, batches, return_all=False):
    """Yield (batch, outputs, loss[, logits, attns, labels]) per batch; a batch is the data module's (x, y, y_len, raw_y) or a
    dict with ``y``, ``y_len`` and further run_model arguments."""
    with torch.no_grad():
        for batch in batches:
            if isinstance(batch, (tuple, list)):
                x, y, y_len, _raw_y = batch
                kwargs = {"x": x}
            elif isinstance(batch, dict):
                kwargs = {k: v for k, v in batch.items() if k not in ("y", "y_len")}
                y, y_len = batch["y"], batch["y_len"]
            else:
                raise TypeError(f"unable to process a batch of type {type(batch).__name__}")
            ret = run_model(model, y, y_len, return_all=return_all, **kwargs)
            yield (batch,) + tuple(t if t is not None else [None] * len(y) for t in ret)


def run_model_on_data(*args, **kwargs):
    """The same per example: (x, y, y_len, raw_y, outputs, loss, ...)."""
    return examples_from_batches((*batch, *ret) for batch, *ret in run_model_on_batches(*args, **kwargs))


def get_model_losses_on_batches(model, batches):
    """-> every utterance's summed loss, one tensor."""
    return torch.cat([loss.sum(-1).detach() for _batch, _outputs, loss in run_model_on_batches(model, batches)], 0)


def build_batch_csr(y, pos_tags, n_cols, key_slots):
    """The CSR cvcl_token_items_accumulate reads, for one batch.  ``y`` [B, L] token ids (host), ``pos_tags`` the B tag lists of
    its utterances, ``n_cols`` the row length of the outputs / loss the row indices refer to (row = b n_cols + l), ``key_slots``
    the running {Key: slot} table, extended in place in visiting order.  Position l of utterance b carries Key(y[b, l], tags[l])
    while l < min(L, len(tags), n_cols) -- a position behind its utterance's tag list has no key, as under the truncating zip of
    the reference (:326).  -> (seg_ptr [S + 1], rows [n_valid], slot [S]) int32: segments in ascending slot order, the rows of a
    segment ascending (a stable sort of the visiting order)."""
    y = np.asarray(y)
    ids, rows = [], []
    for b, tags in enumerate(pos_tags):
        n = min(y.shape[1], len(tags), n_cols)
        for l, (tok, tag) in enumerate(zip(y[b, :n].tolist(), tags)):
            ids.append(key_slots.setdefault(Key(tok, tag), len(key_slots)))
            rows.append(b * n_cols + l)
    ids = np.asarray(ids, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int32)
    order = np.argsort(ids, kind="stable")
    ids, rows = ids[order], rows[order]
    starts = np.flatnonzero(np.concatenate(([True], ids[1:] != ids[:-1]))) if len(ids) else np.zeros(0, dtype=np.int64)
    seg_ptr = np.concatenate((starts, [len(ids)])).astype(np.int32)
    return seg_ptr, rows, ids[starts].astype(np.int32)


class _KeyTables:
    """The running tables on the device, grown by doubling as new keys appear."""

    def __init__(self, hidden_dim, device, capacity=1024):
        self.hidden_dim, self.device = hidden_dim, device
        self._alloc(capacity)

    def _alloc(self, capacity):
        self.vector = torch.zeros(capacity, self.hidden_dim, dtype=torch.float32, device=self.device)
        self.loss = torch.zeros(capacity, dtype=torch.float64, device=self.device)
        self.cnt = torch.zeros(capacity, dtype=torch.int64, device=self.device)

    def reserve(self, n_keys):
        if n_keys <= len(self.cnt):
            return
        old = (self.vector, self.loss, self.cnt)
        self._alloc(max(n_keys, 2 * len(self.cnt)))
        for new, prev in zip((self.vector, self.loss, self.cnt), old):
            new[:len(prev)].copy_(prev)

    def add(self, outputs, loss, csr):
        seg_ptr, rows, slot = (torch.from_numpy(a).to(self.device) for a in csr)
        ops.token_items_accumulate(outputs, loss, seg_ptr, rows, slot, self.vector, self.loss, self.cnt)


def _tagged_batches(runs, pos_tags):
    """(run, its utterances' tag lists) for runs whose first entry is the batch's ``y``; stops with the shorter of the two, like
    the reference's zip over examples."""
    it = iter(pos_tags)
    for item in runs:
        tags = list(itertools.islice(it, len(item[0])))
        if not tags:
            return
        yield item, tags


def get_model_items(model, dataloader, pos_tags, ignore_all_token_items=True):
    """Losses and per-key sums of a language model over a data set (reference :295-344).
    pos_tags: per utterance, the list of its tokens' tags (``<sos>`` and ``<eos>`` included).
    -> ModelItems(losses: per utterance its token losses (numpy, trimmed to its length); all_token_items: None;
    token_pos_items: {Key(token_id, pos): SumData}; token_items: {Key(token_id, majority pos): SumData} with the word's embedding
    row when the model has a ``text_encoder``).  Only ``ignore_all_token_items=True`` is supported: keeping every token's hidden
    vector on the host is what this path exists to avoid.  For an n-gram model the vectors have shape (0,) (the reference's
    hidden_dim = 0; its own n-gram branch reads ``y`` before assigning it, :306) and there is no embedding."""
    if not ignore_all_token_items:
        raise NotImplementedError("all_token_items (one SumData per token on the host) is not kept on the HIP path")
    is_ngram = isinstance(model, ngram.NGramModel)
    if not is_ngram:
        _language_model_of(model)
    device = model.device if is_ngram else get_model_device(model)
    tables = None
    key_slots = {}
    losses_dev, lengths = [], []
    runs = ((*_tokens_of(batch), outputs, loss) for batch, outputs, loss in run_model_on_batches(model, dataloader))
    for (y, y_len, outputs, loss), tags in _tagged_batches(runs, pos_tags):
        n_cols = min(outputs.shape[1], loss.shape[1])        # the LSTM trims its outputs to the batch's longest utterance
        B = len(tags)                                        # (fewer than the batch when the tag lists run out)
        if is_ngram:                                         # cvcl_token_items_accumulate wants H >= 1: one zero column, cut off below
            outputs = outputs.new_zeros(outputs.shape[0], n_cols, 1)
        outputs = outputs[:B, :n_cols].contiguous()
        loss = loss[:B, :n_cols].contiguous()
        if tables is None:
            tables = _KeyTables(outputs.shape[-1], device)
        csr = build_batch_csr(y.cpu().numpy()[:B], tags, n_cols, key_slots)
        tables.reserve(len(key_slots))
        if len(csr[2]):
            tables.add(outputs.reshape(B * n_cols, -1), loss.reshape(-1), csr)
        losses_dev.append(loss)
        lengths.append(y_len.cpu().numpy()[:B])
    losses = []
    for loss, lens in zip(losses_dev, lengths):              # the host copies happen here, after the last launch
        loss = loss.cpu().numpy()
        losses.extend(loss[b, :int(n)] for b, n in enumerate(lens))
    token_pos_items = {}
    if key_slots:
        n = len(key_slots)
        vector, loss_sum, cnt = tables.vector[:n].cpu().numpy(), tables.loss[:n].cpu().numpy(), tables.cnt[:n].cpu().numpy()
        if is_ngram:
            vector = vector[:, :0]
        for key in sorted(key_slots):
            s = key_slots[key]
            token_pos_items[key] = SumData(cnt=np.array(cnt[s]), loss=np.array(loss_sum[s]), vector=vector[s], embedding=None)
    token_items = get_token_items(token_pos_items)
    if hasattr(model, "text_encoder"):
        token_items = update_items_with_embedding(token_items, model.text_encoder.embedding.weight.detach().cpu().numpy())
    return ModelItems(losses, None, token_pos_items, token_items)


def get_token_items(token_pos_items):
    """Merge the (word, tag) items of a word into one item under its majority tag: the tag with the largest count and, among
    equally frequent ones, the LARGER tag string -- max over (cnt, pos), as the reference computes it (:266)."""
    token_items = {}
    ordered = sorted(token_pos_items.items())
    for _token_id, group in itertools.groupby(ordered, key=lambda item: item[0].token_id):
        group = list(group)
        key = max(group, key=lambda item: (int(item[1].cnt), item[0].pos))[0]
        token_items[key] = sum((value for _key, value in group), start=zero_sum_data_like(group[0][1]))
    return token_items


def update_items_with_embedding(items, embedding):
    return {key: value._replace(embedding=embedding[key.token_id]) for key, value in items.items()}


def build_series(items):
    """The reference's pandas form of an items dict: a Series indexed by (token_id, pos), sorted."""
    import pandas as pd
    s = pd.Series(list(items.values()), index=pd.MultiIndex.from_tuples(list(items.keys()), names=Key._fields), dtype=object)
    return s.sort_index()


def build_series_from_pairs(pairs):
    import pandas as pd
    keys, values = zip(*pairs)
    return pd.Series(data=list(values), index=pd.MultiIndex.from_tuples(keys, names=Key._fields), dtype=object)


def _predictions(model, dataloader, pos_tags, top_k, want_probs):
    """Per batch: (index of its first utterance, y host [B, L], tags, label_prob, top_prob, top_idx, probs or None), each
    row-aligned with y (leading zero row for regressional models included)."""
    if isinstance(model, ngram.NGramModel):
        yield from _ngram_predictions(model, dataloader, pos_tags, top_k, want_probs)
        return
    regressional = is_regressional(model)
    runs = ((_tokens_of(batch)[0], ret) for batch, *ret in run_model_on_batches(model, dataloader, return_all=True))
    first = 0
    for (y, (_outputs, _loss, logits, _attns, labels)), tags in _tagged_batches(runs, pos_tags):
        B, Lp, V = logits.shape
        top_prob, top_idx, label_prob, probs = ops.token_topk(logits.reshape(B * Lp, V), labels.reshape(-1), top_k, PAD_TOKEN_ID,
                                                              want_probs)
        top_prob, top_idx, label_prob = top_prob.view(B, Lp, -1), top_idx.view(B, Lp, -1), label_prob.view(B, Lp)
        if probs is not None:
            probs = probs.view(B, Lp, V)
        if regressional:                                     # position 0 predicts nothing: a zero row, whose top-k is 0 .. k - 1
            top_prob = F.pad(top_prob, (0, 0, 1, 0))
            top_idx = torch.cat([torch.arange(top_k, device=top_idx.device).expand(B, 1, top_k), top_idx], 1)
            label_prob = F.pad(label_prob, (1, 0))
            if probs is not None:
                probs = F.pad(probs, (0, 0, 1, 0))
        yield (first, y.cpu().numpy(), tags, label_prob.cpu().numpy(), top_prob.cpu().numpy(), top_idx.cpu().numpy(),
               None if probs is None else probs.cpu().numpy())
        first += len(tags)


def _ngram_predictions(model, dataloader, pos_tags, top_k, want_probs):
    """_predictions for an n-gram model: the rows are calculate_probs' back-off scores (not normalised over the words), with
    the leading zero row.  The ``top_k`` best come from a stable descending sort on the device, which keeps equal scores in
    index order -- torch.topk promises no order among equal values, and words an order has not seen share one score."""
    if not 1 <= top_k <= model.vocab_size:
        raise ValueError(f"top_k {top_k} outside [1, vocab_size = {model.vocab_size}]")
    first = 0
    with torch.no_grad():
        for (y, y_len), tags in _tagged_batches((_tokens_of(batch) for batch in dataloader), pos_tags):
            probs = F.pad(model.calculate_probs(y, y_len, alpha=model.alpha), (0, 0, 1, 0))
            order = torch.sort(probs, dim=-1, descending=True, stable=True)
            labels = y.to(device=probs.device, dtype=torch.int64).clamp(0, model.vocab_size - 1)     # (padding may hold anything)
            label_prob = probs.gather(2, labels.unsqueeze(-1)).squeeze(-1)
            yield (first, torch.as_tensor(y).cpu().numpy(), tags, label_prob.cpu().numpy(), order.values[..., :top_k].cpu().numpy(),
                   order.indices[..., :top_k].cpu().numpy(), probs.cpu().numpy() if want_probs else None)
            first += len(tags)


def _tagged_positions(y, tags, n_cols):
    for b, utterance_tags in enumerate(tags):
        n = min(y.shape[1], len(utterance_tags), n_cols)
        for l in range(n):
            yield b, l, Key(int(y[b, l]), utterance_tags[l])


def get_model_probs(model, dataloader, pos_tags):
    """-> [(Key, probs [V])] per tagged position: the model's distribution over the word AT that position (reference :347-365;
    a zero row at position 0 of regressional models).  The softmax runs on the device; the rows are materialised on the host, as
    in the reference -- get_model_top_predictions avoids that."""
    all_probs = []
    for _first, y, tags, _lp, _tp, _ti, probs in _predictions(model, dataloader, pos_tags, 1, True):
        all_probs.extend((key, probs[b, l]) for b, l, key in _tagged_positions(y, tags, probs.shape[1]))
    return all_probs


def iter_top_predictions(model, dataloader, pos_tags, top_k=5):
    """Yield (utterance, position, Key, label_prob, top_prob [top_k], top_idx [top_k]) per tagged position, the utterances
    numbered through the data set: get_model_top_predictions with the place of every entry beside it."""
    for first, y, tags, label_prob, top_prob, top_idx, _probs in _predictions(model, dataloader, pos_tags, top_k, False):
        for b, l, key in _tagged_positions(y, tags, top_prob.shape[1]):
            yield first + b, l, key, label_prob[b, l], top_prob[b, l], top_idx[b, l]


def get_model_top_predictions(model, dataloader, pos_tags, top_k=5):
    """-> [(Key, label_prob, top_prob [top_k], top_idx [top_k])] per tagged position: the probability the model gave the word at
    that position and its ``top_k`` predictions for it, ordered by (probability desc, index asc).  Only [B, L, top_k] arrays
    reach the host.  Position 0 of a regressional model predicts nothing: probability 0 and the top-k of a zero row."""
    return [entry[2:] for entry in iter_top_predictions(model, dataloader, pos_tags, top_k)]
