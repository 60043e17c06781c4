"""Helpers of the word-level analysis (reference analysis_tools/utils.py: get_model_device, print_top_values)."""
import torch


def get_model_device(model):
    return next(model.parameters()).device


def default_value_formatter(value):
    return f"{value:5.3f}"


def prob_formatter(prob):
    return f"{prob:6.1%}"


def print_top_values(values, idx2word, labels=None, top_k=5, steps=None, value_formatter=default_value_formatter, top=None,
                     label_values=None):
    """One line per step: the label's value (when labels are given), then the ``top_k`` best words with their values
    (reference utils.py:117-150).  ``values`` is a tensor [n_steps, vocab_size] or [vocab_size], as in the reference; or pass
    ``values=None`` with ``top=(top_values, top_indices)`` [n_steps, k] and, beside ``labels``, ``label_values`` [n_steps] --
    what processing.get_model_top_predictions computes on the device, so that no [n_steps, vocab_size] array is needed."""
    if values is not None:
        values = torch.as_tensor(values)
        if values.dim() == 1:
            values = values.unsqueeze(0)
            labels = None if labels is None else torch.as_tensor(labels).reshape(1)
        top_values, top_indices = values.topk(top_k, -1)
        if labels is not None:
            labels = torch.as_tensor(labels)
            label_values = values.gather(1, labels.reshape(-1, 1).to(values.device)).squeeze(1)
    else:
        if top is None:
            raise ValueError("print_top_values: give a value tensor or top=(top_values, top_indices)")
        top_values, top_indices = (torch.as_tensor(t) for t in top)
        if top_values.dim() == 1:
            top_values, top_indices = top_values.unsqueeze(0), top_indices.unsqueeze(0)
        top_values, top_indices = top_values[:, :top_k], top_indices[:, :top_k]
        if labels is not None:
            if label_values is None:
                raise ValueError("print_top_values: labels with a precomputed top-k need label_values")
            labels, label_values = torch.as_tensor(labels).reshape(-1), torch.as_tensor(label_values).reshape(-1)
    n_steps = len(top_values)
    lines = []
    for step in (range(n_steps) if steps is None else steps):
        def fmt(value, idx):
            return f"{value_formatter(float(value))} {idx2word[int(idx)]:8}"
        line = " ".join(fmt(v, i) for v, i in zip(top_values[step], top_indices[step]))
        if labels is not None:
            line = fmt(label_values[step], labels[step]) + " | " + line
        print(line)
        lines.append(line)
    return lines
