"""The reference's image-text alignment analysis (analysis_cvcl/alignment.py, embeddings.py:106-118) on the HIP path
(multimodal/alignment.py)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "multimodal-baby_amd"))

from multimodal import alignment  # noqa: E402

if __name__ == "__main__":
    alignment.main(alignment.parser().parse_args())
