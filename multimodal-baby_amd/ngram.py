"""The back-off n-gram language model of the reference's top-level ngram.py -- the baseline its word-level analysis sets beside
the LSTM -- on the HIP path (csrc/ngram.hip; include/cvcl_hip.h "N-gram baseline").

The reference counts and scores in nested Python loops over dicts keyed by token tuples.  Here an (n + 1)-gram is one
non-negative int64 (its token ids big-endian, ``bits`` each), ``update`` is one cvcl_ngram_keys launch per batch, the counts are
a sorted unique table per order (torch.sort / torch.unique_consecutive on the device: plumbing), and scoring is one
cvcl_ngram_ce_loss or cvcl_ngram_probs launch: two binary searches per back-off step, log and sum in double.  The counts are the
reference's exactly; the losses are its values to the last float32 step.  There is no CPU fallback."""
import math

import torch

from multimodal import _hip as H
from multimodal import ops


def key_bits(vocab_size):
    """Bits one token id takes in a packed key: max(1, bit_length(vocab_size - 1))."""
    return max(1, (int(vocab_size) - 1).bit_length())


def _reduce(keys, counts):
    """Sorted keys with a count each -> (distinct keys, the sum of the counts of each): exact integer sums in a fixed order."""
    uk, run = torch.unique_consecutive(keys, return_counts=True)
    total = counts.cumsum(0)[run.cumsum(0) - 1]
    return uk, torch.diff(total, prepend=total.new_zeros(1))


class NGramModel:
    """``NGramModel(N, vocab_size, device=None)``: the reference's surface (``N``, ``update``, ``calculate_ce_loss``) plus
    ``calculate_probs`` and ``to_counts``.  1 <= N <= 8 and N * key_bits(vocab_size) <= 63 (vocab_size 2350: N <= 5), else
    ValueError.  ``device`` defaults to the current HIP device.  ``alpha`` (an attribute, 0.1 at construction; not in the
    reference) is the smoothing weight analysis_tools.processing scores with, since its functions take a model and no alpha:
    set it before handing the model over (word_statistics.py --ngram_alpha does).  The methods' own ``alpha`` arguments do not
    read it.

    Inputs may live on the CPU, have another integer dtype or be non-contiguous: they are moved and converted on the host.
    Results live on the MODEL's device (the reference returns on ``y``'s device).  A token id outside [0, vocab_size) inside an
    utterance's length raises ValueError (the reference would count or look up the id as it is)."""

    def __init__(self, N, vocab_size, device=None):
        if int(N) != N or not 1 <= N <= H.NGRAM_MAX_N:
            raise ValueError(f"N-gram model requires 1 <= N <= {H.NGRAM_MAX_N}, got {N}")
        if int(vocab_size) != vocab_size or vocab_size < 1:
            raise ValueError(f"vocab_size {vocab_size} < 1")
        self._N, self._vocab_size, self._bits = int(N), int(vocab_size), key_bits(vocab_size)
        if self._N * self._bits > 63:
            raise ValueError(f"N {N} x {self._bits} bits per token (vocab_size {vocab_size}) does not fit the 63 key bits")
        self.alpha = 0.1                                     # the alpha analysis_tools.processing scores with
        self._device = None if device is None else torch.device(device)
        self._pending = []                                   # [N, B L] key tensors of the updates since the last rebuild
        self._gram = [None] * self._N                        # per order (keys, counts), sorted; None = nothing counted
        self._tables = None

    @property
    def N(self):
        return self._N

    @property
    def vocab_size(self):
        return self._vocab_size

    @property
    def device(self):
        if self._device is None or (self._device.type == "cuda" and self._device.index is None):
            if not torch.cuda.is_available():
                raise H.CvclError("the n-gram model runs on the HIP path: no GPU, and there is no CPU fallback")
            self._device = torch.device("cuda", torch.cuda.current_device())
        return self._device

    # ---- host plumbing
    def _inputs(self, y, y_len):
        if (self._device is not None and self._device.type != "cuda") or not torch.cuda.is_available():
            raise H.CvclError("the n-gram model runs on the HIP path: no GPU, and there is no CPU fallback")
        y, y_len = torch.as_tensor(y), torch.as_tensor(y_len)
        if y.dim() != 2 or y_len.dim() != 1 or len(y_len) != len(y) or y.is_floating_point() or y_len.is_floating_point():
            raise ValueError(f"y [B, L] and y_len [B] of integers are needed, got {tuple(y.shape)} and {tuple(y_len.shape)}")
        dev = self.device
        return (y.to(device=dev, dtype=torch.int64).contiguous(), y_len.to(device=dev, dtype=torch.int64).contiguous())

    def _refuse_bad_ids(self, bad, what):
        n = int(bad.item())                                  # the one 4-byte copy
        if n:
            raise ValueError(f"{what}: {n} token id(s) outside [0, {self._vocab_size}) inside the utterance lengths")

    @staticmethod
    def _alpha(alpha):
        if not 0.0 < alpha < 1.0:
            raise ValueError(f"alpha {alpha} outside (0, 1)")
        return math.log(alpha), math.log(1 - alpha)

    def _rebuild(self):
        """The tables of all orders in cvcl_hip.h's layout, from the old (keys, counts) and the keys appended since."""
        if self._tables is not None:
            return self._tables
        if self._pending:
            with torch.cuda.device(self.device):
                for n in range(self._N):
                    keys = torch.sort(torch.cat([p[n] for p in self._pending])).values
                    keys, counts = torch.unique_consecutive(keys, return_counts=True)
                    keep = keys != H.NGRAM_SENTINEL              # the sentinel sorts first: at most the leading entry goes
                    keys, counts = keys[keep], counts[keep]
                    if self._gram[n] is not None:
                        keys, order = torch.sort(torch.cat([self._gram[n][0], keys]))
                        keys, counts = _reduce(keys, torch.cat([self._gram[n][1], counts])[order])
                    self._gram[n] = (keys, counts) if keys.numel() else None
            self._pending = []
        dev = self.device
        empty = torch.zeros(0, dtype=torch.int64, device=dev)
        grams = [g if g is not None else (empty, empty) for g in self._gram]
        ctxs = [_reduce(k >> self._bits, c) if k.numel() else (empty, empty) for k, c in grams]
        offsets = lambda tabs: [0] + torch.tensor([len(k) for k, _c in tabs]).cumsum(0).tolist()       # noqa: E731
        self._tables = (torch.cat([k for k, _c in grams]), torch.cat([c for _k, c in grams]), offsets(grams),
                        torch.cat([k for k, _c in ctxs]), torch.cat([c for _k, c in ctxs]), offsets(ctxs))
        return self._tables

    # ---- the reference's surface
    def update(self, y, y_len):
        """Count the batch's utterances (reference ngram.py:20-36): y [B, L] token ids, every utterance starting with <sos>,
        y_len [B].  One launch; the tables are rebuilt on the next scoring call.  Several updates equal one update on the
        concatenated data."""
        y, y_len = self._inputs(y, y_len)
        B, L = y.shape
        if B == 0 or L < 2:
            return                                           # position 0 is never predicted: nothing to count
        with torch.cuda.device(self.device):
            keys, bad = ops.ngram_keys(y, y_len, self._N, self._vocab_size)
            self._refuse_bad_ids(bad, "update")
        self._pending.append(keys.view(self._N, B * L))
        self._tables = None

    def calculate_ce_loss(self, y, y_len, alpha=0.1, tokenwise=True):
        """The cross-entropy losses (reference ngram.py:38-79) -> loss [B, L - 1] float32 on the model's device, zeros outside
        the utterances; ``tokenwise=False``: their sum over the number of scored tokens, a device scalar (NaN when no token is
        scored, as the reference's 0 / 0).  ``alpha`` in (0, 1) is the share left to the lower orders.  A model that has counted
        nothing raises Exception("Even unigram is not applicable.") -- always, where the reference raises only if at least one
        token is to be scored: the table sizes are on the host, the lengths are not."""
        log_alpha, log_1m_alpha = self._alpha(alpha)
        y, y_len = self._inputs(y, y_len)
        tables = self._rebuild()
        if tables[2][1] == 0:
            raise Exception("Even unigram is not applicable.")
        B, L = y.shape
        if B == 0 or L < 2:
            loss = torch.zeros(B, 0, dtype=torch.float32, device=self.device)
        else:
            with torch.cuda.device(self.device):
                loss, bad = ops.ngram_ce_loss(tables, self._N, self._vocab_size, log_alpha, log_1m_alpha, y, y_len)
                self._refuse_bad_ids(bad, "calculate_ce_loss")
        if not tokenwise:
            n_tokens = (y_len.clamp(0, L) - 1).clamp_min(0).sum()
            return loss.sum() / n_tokens
        return loss

    def calculate_probs(self, y, y_len, alpha=0.1):
        """-> probs [B, L - 1, vocab_size] float32: exp(-loss) the model would give EVERY word at each position, zero rows
        outside the utterances.  These are the back-off scores of calculate_ce_loss; they are not normalised over the words."""
        log_alpha, log_1m_alpha = self._alpha(alpha)
        y, y_len = self._inputs(y, y_len)
        tables = self._rebuild()
        if tables[2][1] == 0:
            raise Exception("Even unigram is not applicable.")
        B, L = y.shape
        if B == 0 or L < 2:
            return torch.zeros(B, max(L - 1, 0), self._vocab_size, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            probs, bad = ops.ngram_probs(tables, self._N, self._vocab_size, log_alpha, log_1m_alpha, y, y_len)
            self._refuse_bad_ids(bad, "calculate_probs")
        return probs

    def to_counts(self):
        """The reference's ``_count``: per order n a dict {context tuple of n ids: [total, {word: count}]}, host ints."""
        if (self._device is not None and self._device.type != "cuda") or not torch.cuda.is_available():
            raise H.CvclError("the n-gram model runs on the HIP path: no GPU, and there is no CPU fallback")
        gram_key, gram_cnt, gram_off, _ck, _ct, _co = self._rebuild()
        keys, cnts = gram_key.cpu().tolist(), gram_cnt.cpu().tolist()
        mask = (1 << self._bits) - 1
        out = []
        for n in range(self._N):
            table = {}
            for key, c in zip(keys[gram_off[n]:gram_off[n + 1]], cnts[gram_off[n]:gram_off[n + 1]]):
                ctx = tuple((key >> (self._bits * (n - j))) & mask for j in range(n))
                entry = table.setdefault(ctx, [0, {}])
                entry[0] += c
                entry[1][key & mask] = c
            out.append(table)
        return out
