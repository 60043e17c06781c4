"""The reference's train / eval nearest-neighbour checks (analysis_cvcl/duplicates.py) on the HIP path (multimodal/neighbors.py)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "multimodal-baby_amd"))

from multimodal import neighbors  # noqa: E402

if __name__ == "__main__":
    neighbors.main(neighbors.parser().parse_args())
