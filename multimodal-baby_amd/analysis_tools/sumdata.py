"""``SumData``: the running (count, loss, vector, embedding) record of a word (the interface of the reference's
analysis_tools/sumdata.py).  The sums themselves are formed on the device (cvcl_token_items_accumulate); this is the host record
the tables are unpacked into, with the reference's derived values and its + / - for regrouping keys."""
from typing import NamedTuple

import numpy as np

PPL_CAP = 99999.99


def _host(v):
    return v.detach().cpu().numpy() if hasattr(v, "detach") else v


class SumData(NamedTuple):
    cnt: object
    loss: object
    vector: object
    embedding: object = None

    @property
    def mean_vector(self):
        return self.vector / np.expand_dims(self.cnt, -1)

    @property
    def mean_loss(self):
        return self.loss / self.cnt

    @property
    def ppl(self):
        return min(np.exp(self.mean_loss), PPL_CAP)

    def _combine(self, other, sign):
        return SumData(self.cnt + sign * other.cnt, self.loss + sign * other.loss, self.vector + sign * other.vector, self.embedding)

    def __add__(self, other):                            # the left operand's embedding is kept
        return self._combine(other, 1)

    def __sub__(self, other):
        return self._combine(other, -1)

    def to_numpy(self):
        return SumData(self.cnt, self.loss, _host(self.vector), None if self.embedding is None else _host(self.embedding))


def zero_sum_data(hidden_dim, shape=()):
    shape = tuple(shape)
    return SumData(np.zeros(shape, dtype=int), np.zeros(shape), np.zeros(shape + (hidden_dim,)), None)


def zero_sum_data_like(sum_data):
    return zero_sum_data(np.shape(sum_data.vector)[-1], shape=np.shape(sum_data.cnt))
