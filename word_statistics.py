"""The reference's per-word language-model analysis (analysis_tools/processing.py: get_model_items, get_model_probs) on the HIP
path (analysis_tools/word_statistics.py)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "multimodal-baby_amd"))

from analysis_tools import word_statistics  # noqa: E402

if __name__ == "__main__":
    word_statistics.main(word_statistics.parser().parse_args())
