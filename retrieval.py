"""Image <-> text retrieval of a CVCL model over a split's (frame, utterance) pairs: Recall@K, median / mean rank, MRR in both
directions on the HIP path (multimodal/retrieval.py).

    python retrieval.py [--checkpoint PATH | --random_init] (--dataset synthetic | --data_dir DIR [--frame_store PATH])
                        --split val|test [--ks 1 5 10] [--precision 32|32-split] [--chunk N] [--save_features] [--out DIR]
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "multimodal-baby_amd"))

from multimodal import retrieval  # noqa: E402

if __name__ == "__main__":
    retrieval.main(retrieval.parser().parse_args())
