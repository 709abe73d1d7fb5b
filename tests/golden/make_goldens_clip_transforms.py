"""
Generates tests/golden/clip_transforms.npz in the BUILD container from the reference's coclr_utils/transforms.py:
    python tests/golden/make_goldens_clip_transforms.py
torchvision is not installed, so a shim provides the two names the module uses (transforms.Lambda, transforms.Compose), as
make_goldens_classifier.py does for coclr_utils/utils.py.  The cases are tests/clip_transforms_cases.py.  Per case:
    in_<key>        the input (stored once per key)
    seed_<case>     the s of random.seed(s); np.random.seed(s) before the call
    out_<case>      the reference's output (CPU, fp32)
    next_<case>     (random.random(), np.random.uniform()) drawn right after the call: the draw-count check
    dev_<case>      gated cases only: max |fp32 output - the same chain in float64| (same seed; the to-float step patched to float64)

One function of the reference cannot be pinned as it stands.  random_grayscale(vid, factor, channel=1) hands its FRAME axis to
rgb_to_grayscale as the colour axis: the call asserts unless the clip has exactly three frames, and then weights frames instead of
colours.  The package builds what the function evidently means (the luma of each drawn frame over its colour channels), so for the
RandomGray cases this generator replaces the function by `random_grayscale_over_colour` below — the reference's draw, its
rgb_to_grayscale on the colour axis, its blend.
"""
import os
import random
import sys
import types
sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import clip_transforms_cases as cases                      # noqa: E402


class Lambda:
    def __init__(self, lambd):
        self.lambd = lambd

    def __call__(self, x):
        return self.lambd(x)


class Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


def random_grayscale_over_colour(R):
    def fn(vid, factor, channel=1):
        drawn = np.random.uniform(size=(vid.size(channel),)) < factor
        if drawn.sum() == 0:
            return vid
        m = torch.tensor(drawn).float().view(1, -1, 1, 1)
        return R.rgb_to_grayscale(vid, 0).unsqueeze(0) * m + vid * (1 - m)
    return fn


def seed(s):
    random.seed(s)
    np.random.seed(s)


def main():
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.transforms.Lambda, tv.transforms.Compose = Lambda, Compose
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tv.transforms)
    sys.path.insert(0, "/root/reference")
    import coclr_utils.transforms as R                      # the reference

    R.random_grayscale = random_grayscale_over_colour(R)
    ins = cases.inputs()
    out = {f"in_{k}": v for k, v in ins.items()}
    to01, to255 = R.to_normalized_float_tensor, R.to_float_tensor
    for name, key, s, kind, build in cases.CASES:
        x = ins[key]
        seed(s)
        y = cases.run_case(build, R, Compose, Lambda, key, x)
        nxt = np.array([random.random(), np.random.uniform()])
        assert y.dtype == torch.float32
        out[f"seed_{name}"], out[f"out_{name}"], out[f"next_{name}"] = np.int64(s), y.numpy().copy(), nxt
        if kind != "eq":
            R.to_normalized_float_tensor = lambda vid: vid.permute(3, 0, 1, 2).to(torch.float64) / 255
            R.to_float_tensor = lambda vid: vid.permute(3, 0, 1, 2).to(torch.float64)
            try:
                seed(s)
                y64 = cases.run_case(build, R, Compose, Lambda, key, x if x.dtype == np.uint8 else x.astype(np.float64))
            finally:
                R.to_normalized_float_tensor, R.to_float_tensor = to01, to255
            assert y64.dtype == torch.float64 and y64.shape == y.shape
            out[f"dev_{name}"] = np.float64((y.double() - y64).abs().max().item())
            print(f"  {name}: shape {tuple(y.shape)}, fp32 vs fp64 {out[f'dev_{name}']:.3e}")
        else:
            print(f"  {name}: shape {tuple(y.shape)}")
    path = os.path.join(HERE, "clip_transforms.npz")
    np.savez_compressed(path, **out)
    print("clip transform goldens:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
