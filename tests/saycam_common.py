"""The tiny SAYCam-layout dataset shared by tools/gen_golden_saycam_data.py and the SAYCam / frame-store tests.

``metadata()`` is the dataset's description (what tests/golden/saycam_data.json holds): the pair splits and the evaluation
trial lists, evaluation frames by paths relative to the data directory.  ``materialize(dir, meta)`` writes it to disk in the
reference's layout, every frame regenerated from a seed derived from its name (train frames JPEG, evaluation frames PNG)."""
import json
import os
import zlib

import numpy as np

H = W = 224
CATEGORIES = ("ball", "car", "cat", "dog")
LONG = " ".join(["look at the ball and the car and the dog"] * 3)          # 30 words: 32 tokens with <sos> / <eos>, over the 25 kept


def metadata():
    frames = [f"clip{i // 4}_{i % 4:02d}.jpg" for i in range(12)]
    train = [{"utterance": "look at the ball", "frame_filenames": frames[0:1]},
             {"utterance": "you want to see the zzyzx kitty", "frame_filenames": frames[1:5]},          # zzyzx: not in the vocabulary
             {"utterance": LONG, "frame_filenames": frames[5:7]},
             {"utterance": "yeah", "frame_filenames": frames[7:8]},
             {"utterance": "we can read this book one more time", "frame_filenames": frames[8:11]},
             {"utterance": "okay go play with it now", "frame_filenames": frames[11:12]}]
    utterances = [d["utterance"] for d in train]
    shuffled = [{"utterance": utterances[(i + 2) % len(train)], "frame_filenames": d["frame_filenames"]} for i, d in enumerate(train)]
    val = [{"utterance": "here is your little car", "frame_filenames": frames[2:4]},
           {"utterance": "that is a dog", "frame_filenames": frames[9:10]},
           {"utterance": "and there it is", "frame_filenames": frames[6:7]}]
    test = [{"utterance": "the cat", "frame_filenames": frames[4:5]},
            {"utterance": "look a ball qqqq", "frame_filenames": frames[10:12]},
            {"utterance": "more", "frame_filenames": frames[0:2]}]
    out = {"train.json": {"data": train}, "train_shuffled.json": {"data": shuffled}, "val.json": {"data": val},
           "test.json": {"data": test}}
    for stage in ("dev", "test"):
        trials = []
        for t, cat in enumerate(CATEGORIES):
            foils = [CATEGORIES[(t + k) % 4] for k in (1, 2, 3)]
            trials.append({"target_category": cat, "foil_categories": foils,
                           "target_img_filename": f"eval/{stage}/{cat}/img_{t % 2}.png",
                           "foil_img_filenames": [f"eval/{stage}/{f}/img_{(t + k) % 2}.png" for k, f in enumerate(foils)]})
        out[f"eval_{stage}.json"] = {"data": trials}
    return out


def frame_pixels(name, h=H, w=W):
    """uint8 [h, w, 3]: coloured 16 x 16 blocks plus noise, seeded by the frame's name"""
    rng = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    coarse = rng.randint(0, 256, (-(-h // 16), -(-w // 16), 3))
    img = np.kron(coarse, np.ones((16, 16, 1), dtype=np.int64))[:h, :w]
    return np.clip(img + rng.randint(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)


def frame_names(meta):
    """(train frame names, evaluation frame paths), each sorted"""
    train = sorted({n for k in ("train.json", "train_shuffled.json", "val.json", "test.json") for d in meta[k]["data"]
                    for n in d["frame_filenames"]})
    ev = sorted({n for k in meta if k.startswith("eval_") for t in meta[k]["data"]
                 for n in [t["target_img_filename"]] + t["foil_img_filenames"]})
    return train, ev


def materialize(root, meta):
    from PIL import Image
    root = str(root)
    os.makedirs(os.path.join(root, "train_5fps"), exist_ok=True)
    for name, content in meta.items():
        with open(os.path.join(root, name), "w") as f:
            json.dump(content, f)
    train, ev = frame_names(meta)
    for n in train:
        Image.fromarray(frame_pixels(n)).save(os.path.join(root, "train_5fps", n), quality=90)
    for n in ev:
        os.makedirs(os.path.dirname(os.path.join(root, n)), exist_ok=True)
        Image.fromarray(frame_pixels(n)).save(os.path.join(root, n))
    return root


def load_committed_metadata(golden_dir):
    with open(os.path.join(golden_dir, "saycam_data.json")) as f:
        return json.load(f)
