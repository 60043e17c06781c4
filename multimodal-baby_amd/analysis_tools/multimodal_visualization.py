"""The reference's import path for the per-model visualisation calls (reference analysis_tools/multimodal_visualization.py):
``gradCAM_for_captioning_lm`` is multimodal.attention_maps' batched HIP path called on one image and one caption,
``torch_to_numpy_image`` the [C, H, W] -> [H, W, C] host copy the plotting helpers expect."""
from multimodal.attention_maps import gradCAM_for_captioning_lm

__all__ = ["torch_to_numpy_image", "gradCAM_for_captioning_lm", "attention_for_attention_lm"]


def torch_to_numpy_image(img):
    """[C, H, W] tensor (any device) -> [H, W, C] numpy array."""
    return img.detach().permute(1, 2, 0).cpu().numpy()


def attention_for_attention_lm(model, x, y, y_len, steps=None):
    raise NotImplementedError("attention language models are outside the implemented path")
