"""The cases of tests/golden/clip_transforms.npz, shared by the generator (which builds each chain from the reference's module)
and the tests (which build it from video_similarity_search_amd.coclr_utils.transforms): the class and function names are the same.

A case is (name, input key, seed, gate, build).  build(T, C, L) returns the chain: T is the transforms module, C a Compose
constructor, L the Lambda class that wraps a plain function call.  gate: "eq" = bit equality; "dev" = 4 x the stored fp32-vs-fp64
deviation of the reference, floored at 2^-23 (unit-range data); "dev/std" = that floor divided by min(std) (after Normalize).
Input keys ending in "_batch" are run clip by clip and stacked (the reference) / through Compose.batch (this package)."""
import numpy as np
import torch

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
FLOOR = 2.0 ** -23


def inputs():
    rng = np.random.default_rng(20240607)
    u13 = rng.integers(0, 256, (3, 13, 19, 3), dtype=np.uint8)
    u13[0, 0, 0], u13[2, 12, 18] = (0, 255, 0), (255, 0, 255)                 # both ends of the range, on corners
    return {
        "u13": u13,
        "u5": rng.integers(0, 256, (5, 13, 19, 3), dtype=np.uint8),           # five frames: per-frame factors
        "u70": rng.integers(0, 256, (2, 70, 90, 3), dtype=np.uint8),          # contrast: more pixels than one workgroup reduces
        "us": rng.integers(0, 256, (2, 9, 11, 3), dtype=np.uint8),            # the many-seed cases
        "f13": rng.random((3, 3, 13, 19), dtype=np.float32),
        "fs": rng.random((3, 2, 5, 7), dtype=np.float32),
        "f5d": rng.random((2, 3, 4, 6, 5), dtype=np.float32),                 # [B, 3, N, H, W]
        "u13_batch": rng.integers(0, 256, (3, 3, 13, 19, 3), dtype=np.uint8),
    }


def f64(*v):
    return torch.tensor(v, dtype=torch.float64)


def _bench_chain(T, C, size):
    return C([T.ToFloatTensorInZeroOne(), T.RandomSizedCrop(size), T.RandomHorizontalFlip(),
              T.ColorJitter(0.4, 0.4, 0.4, consistent=True), T.RandomGray(0.2), T.Normalize(MEAN, STD)])


CASES = [
    ("tofloat01", "u13", 1, "eq", lambda T, C, L: C([T.ToFloatTensorInZeroOne()])),
    ("tofloat", "u13", 1, "eq", lambda T, C, L: C([T.ToFloatTensor()])),
    ("crop_edge", "u13", 1, "eq", lambda T, C, L: C([T.ToFloatTensorInZeroOne(), L(lambda v: T.crop(v, 4, 6, 9, 13))])),
    ("center_crop", "u13", 1, "eq", lambda T, C, L: C([T.ToFloatTensorInZeroOne(), T.CenterCrop((8, 10))])),     # round(2.5) = 2
    ("random_crop", "u13", 2, "eq", lambda T, C, L: C([T.ToFloatTensor(), T.RandomCrop((7, 11))])),
    ("random_crop_same", "f13", 2, "eq", lambda T, C, L: C([T.RandomCrop((13, 19)), T.Normalize(MEAN, STD)])),     # no draw
    ("flip", "f13", 3, "eq", lambda T, C, L: C([T.RandomHorizontalFlip(p=1.0)])),
    ("flip_maybe", "u13", 4, "eq", lambda T, C, L: C([T.ToFloatTensorInZeroOne(), T.RandomHorizontalFlip()])),
    ("flip_maybe2", "u13", 5, "eq", lambda T, C, L: C([T.ToFloatTensorInZeroOne(), T.RandomHorizontalFlip()])),
    ("pad", "u13", 1, "eq", lambda T, C, L: C([T.ToFloatTensor(), T.Pad((1, 2, 3, 4), fill=7.5)])),
    ("pad_crop_flip", "u13", 1, "eq", lambda T, C, L: C([T.ToFloatTensorInZeroOne(), T.Pad((1, 2, 3, 4), fill=0.25),
                                                        L(lambda v: T.crop(v, 2, 0, 15, 20)), L(T.hflip)])),
    ("normalize", "f13", 1, "eq", lambda T, C, L: C([T.Normalize(MEAN, STD)])),
    ("brightness", "f13", 1, "eq", lambda T, C, L: C([L(lambda v: T.adjust_brightness(v, f64(1.9, 0.3, 1.0)))])),    # 1.9 saturates
    ("brightness_255", "u13", 1, "eq", lambda T, C, L: C([T.ToFloatTensor(), L(lambda v: T.adjust_brightness(v, f64(0.5, 0.001, 1.0)))])),
    ("saturation", "f13", 1, "eq", lambda T, C, L: C([L(lambda v: T.adjust_saturation(v, f64(0.0, 1.7, 0.6)))])),
    ("gray_some", "u5", 3, "eq", lambda T, C, L: C([T.ToFloatTensorInZeroOne(), T.RandomGray(0.5)])),
    ("gray_none", "f13", 1, "eq", lambda T, C, L: C([T.RandomGray(0.0)])),
    ("chain_eq", "u13", 7, "eq", lambda T, C, L: C([T.ToFloatTensorInZeroOne(), L(lambda v: T.crop(v, 1, 2, 11, 15)), T.Pad((2, 1, 0, 3), fill=0.5),
                                                   T.RandomHorizontalFlip(p=1.0), T.ColorJitter(brightness=0.9, saturation=0.4),
                                                   T.RandomGray(0.5), T.Normalize(MEAN, STD)])),
    ("colour_then_geometry", "f13", 1, "eq", lambda T, C, L: C([L(lambda v: T.adjust_brightness(v, f64(1.2, 0.8, 1.0))),
                                                               T.RandomHorizontalFlip(p=1.0), L(lambda v: T.crop(v, 3, 5, 6, 9))])),
    ("contrast", "u70", 1, "dev", lambda T, C, L: C([T.ToFloatTensorInZeroOne(), L(lambda v: T.adjust_contrast(v, f64(0.6, 1.4)))])),
    ("two_contrasts", "f13", 1, "dev", lambda T, C, L: C([L(lambda v: T.adjust_contrast(v, f64(0.6, 1.4, 1.0))),
                                                        L(lambda v: T.adjust_contrast(v, f64(1.3, 0.2, 0.9)))])),
    ("resize_down", "u13", 1, "dev", lambda T, C, L: C([T.ToFloatTensorInZeroOne(), L(lambda v: T.crop(v, 4, 6, 9, 13)), T.Resize((8, 10))])),
    ("resize_up", "u13", 1, "dev", lambda T, C, L: C([T.ToFloatTensorInZeroOne(), L(lambda v: T.crop(v, 4, 6, 9, 13)), T.Resize((20, 27))])),
    ("resize_factor", "u13", 1, "dev", lambda T, C, L: C([T.ToFloatTensorInZeroOne(), L(lambda v: T.crop(v, 4, 6, 9, 13)), T.Resize(7)])),
    ("pad_then_resize", "u13", 1, "dev", lambda T, C, L: C([T.ToFloatTensorInZeroOne(), T.Pad((1, 2, 3, 4), fill=0.5), T.Resize((10, 12))])),
    ("flip_resize_float", "f13", 1, "dev", lambda T, C, L: C([T.RandomHorizontalFlip(p=1.0), T.Resize((8, 10)), T.CenterCrop((6, 7))])),
    ("two_resizes", "u13", 1, "dev", lambda T, C, L: C([T.ToFloatTensorInZeroOne(), T.Resize((8, 10)), T.Resize((12, 9))])),
    ("jitter_per_frame", "u5", 11, "dev/std", lambda T, C, L: C([T.ToFloatTensorInZeroOne(), T.ColorJitter(0.4, 0.4, 0.4, consistent=False),
                                                               T.Normalize(MEAN, STD)])),
    ("sized_crop_factor", "us", 5, "dev", lambda T, C, L: C([T.ToFloatTensorInZeroOne(), T.RandomSizedCrop(6)])),
    ("flip_norm_5d", "f5d", 1, "eq", lambda T, C, L: C([T.RandomHorizontalFlip(p=1.0), T.Normalize(MEAN, STD, channel=1)])),
    ("batch_eq", "u13_batch", 21, "eq", lambda T, C, L: C([T.ToFloatTensorInZeroOne(), T.RandomCrop((9, 12)), T.RandomHorizontalFlip(),
                                                         T.ColorJitter(brightness=0.5, saturation=0.5), T.Normalize(MEAN, STD)])),
    ("batch_bench", "u13_batch", 22, "dev/std", lambda T, C, L: _bench_chain(T, C, (8, 10))),
]
CASES += [(f"jitter_s{s}", "fs", s, "dev", lambda T, C, L: C([T.ColorJitter(0.4, 0.4, 0.4, consistent=True)])) for s in range(12)]
CASES += [(f"bench_s{s}", "us", s, "dev/std", lambda T, C, L: _bench_chain(T, C, (8, 10))) for s in range(30, 33)]


def run_case(build, T, C, L, key, x, device="cpu"):
    """the case's output for input array x, with the generators as the caller seeded them"""
    chain = build(T, C, L)
    t = torch.from_numpy(x).to(device)
    if key.endswith("_batch"):
        return chain.batch(t) if hasattr(chain, "batch") else torch.stack([chain(c) for c in t])
    return chain(t)


def gate(kind, dev):
    """largest allowed |difference| of a "dev" case"""
    floor = FLOOR / min(STD) if kind == "dev/std" else FLOOR
    return max(4.0 * float(dev), floor)
