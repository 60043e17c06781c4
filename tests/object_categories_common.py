"""A tiny object-category dataset on disk for the object-category tests: 5 folders named with vocabulary words (one of them "cat"),
one folder whose name is no word, 3 JPEGs each of mixed sizes, written with Pillow from seeded numpy.  Every category has its own
colour and stripe pattern, so that an image encoder does not see 18 alike frames.  Nothing here touches the GPU or the package."""
import os

import numpy as np

CATEGORIES = ["ball", "car", "cat", "dog", "shoe"]       # sorted; all in multimodal/vocab.json, as is "kitty"
NOT_A_WORD = "zzzunknownthing"
SIZES = [(37, 53), (224, 224), (300, 200)]               # (width, height) of a category's three files
N_TRIALS = len(CATEGORIES) * len(SIZES) * 5


def frame_pixels(category_index, file_index, width, height):
    """uint8 [height, width, 3]: a base colour and stripes whose direction and period are the category's, plus seeded noise"""
    rng = np.random.RandomState(1000 * category_index + file_index)
    base = np.array([[230, 40, 40], [40, 200, 60], [40, 60, 230], [220, 210, 30], [200, 40, 210], [128, 128, 128]][category_index])
    y, x = np.mgrid[0:height, 0:width]
    phase = (x * (category_index + 1) + y * (5 - category_index)) * (2 * np.pi / max(width, height)) * (2 + category_index)
    stripes = 0.5 + 0.5 * np.sin(phase)
    img = base[None, None, :] * (0.25 + 0.75 * stripes[..., None]) + rng.randint(-12, 13, size=(height, width, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def materialize(root, empty=None):
    """write the dataset under ``root`` -> its path; ``empty``: a category whose folder is left without files"""
    from PIL import Image
    root = str(root)
    for ci, cat in enumerate(CATEGORIES + [NOT_A_WORD]):
        folder = os.path.join(root, "object_categories", cat)
        os.makedirs(folder, exist_ok=True)
        if cat == empty:
            continue
        for fi, (w, h) in enumerate(SIZES):
            Image.fromarray(frame_pixels(ci, fi, w, h)).save(os.path.join(folder, f"{cat}_{fi:02d}.jpg"), quality=92)
    with open(os.path.join(root, "object_categories", "README.txt"), "w") as f:      # a plain file beside the folders: not a category
        f.write("object categories\n")
    return root
