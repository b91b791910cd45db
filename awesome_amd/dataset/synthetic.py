"""Deterministic synthetic inputs for the BASELINE configs.  No files, no network.

The reference's datasets (SISBOSI / FBMS-59, awesome/dataset/*) need data that is not on disk; the hot path only needs
per-image unaries in [0,1] with the reference's convention fg = 0, bg = 1 (notebooks/how_to/convexity.ipynb cell 7,
awesome/model/path_connected_net.py:832-836)."""
from __future__ import annotations

import numpy as np
import torch


def _convex_hull(pts: np.ndarray) -> np.ndarray:
    """Andrew monotone chain; returns hull vertices counter-clockwise."""
    pts = pts[np.lexsort((pts[:, 1], pts[:, 0]))]

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])

    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in pts[::-1]:
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return np.asarray(lower[:-1] + upper[:-1])


def convex_blob_mask(size: int = 256, seed: int = 0, n_vertices: int = 8) -> np.ndarray:
    """C2 'convex blob': convex hull of K vertices at sorted random angles, radii U(40,90)/256*size around a centre
    U(96,160)/256*size, rasterised by half-plane tests.  Returns a bool (size,size) mask (True = object)."""
    rng = np.random.RandomState(seed)
    s = size / 256.0
    ang = np.sort(rng.uniform(0.0, 2.0 * np.pi, n_vertices))
    rad = rng.uniform(40.0, 90.0, n_vertices) * s
    cx, cy = rng.uniform(96.0, 160.0, 2) * s
    pts = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1)
    hull = _convex_hull(pts)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    inside = np.ones((size, size), dtype=bool)
    for i in range(len(hull)):
        a, b = hull[i], hull[(i + 1) % len(hull)]
        inside &= ((b[0] - a[0]) * (yy - a[1]) - (b[1] - a[1]) * (xx - a[0])) >= 0.0
    return inside


def convex_blob_unaries(size: int = 256, seed: int = 0) -> torch.Tensor:
    """(size,size) float32 unaries, fg (object) = 0, bg = 1."""
    return torch.from_numpy(1.0 - convex_blob_mask(size, seed).astype(np.float32))


def noisy_blob_unaries(size: int = 256, seed: int = 0, flip_p: float = 0.1, n_squares: int = 3, square: int = 8) -> torch.Tensor:
    """C5 'UNet-logit refinement' input: the C2 blob as pseudo-labels with every pixel flipped w.p. flip_p plus
    n_squares random false-positive squares, turned into synthetic segmentation logits `+-2 + N(0,1)` (object positive);
    unaries = 1 - sigmoid(logit): soft values in (0,1), fg ~ 0 - what a segmentation backbone hands to the prior fit."""
    rng = np.random.RandomState(10_000 + seed)
    m = convex_blob_mask(size, seed)
    lab = m ^ (rng.uniform(size=m.shape) < flip_p)
    s = max(1, int(round(square * size / 256.0)))
    for _ in range(n_squares):
        y, x = rng.randint(0, size - s, 2)
        lab[y:y + s, x:x + s] = True
    logit = np.where(lab, 2.0, -2.0) + rng.normal(size=m.shape)
    return torch.from_numpy((1.0 - 1.0 / (1.0 + np.exp(-logit))).astype(np.float32))


def disc_unaries(h: int, w: int, cy: float, cx: float, r: float) -> torch.Tensor:
    """C1 disc: fg = 0 inside the disc, bg = 1."""
    yy, xx = np.mgrid[0:h, 0:w]
    disc = ((yy - cy) ** 2 + (xx - cx) ** 2) <= r * r
    return torch.from_numpy(1.0 - disc.astype(np.float32))


def star_shape(seed: int = 0):
    """The seeded parameters of the `star` kind in grid coordinates ([0, 1]^2): (cx, cy, r0, a, k, phase) of the region
    |x - c| <= r0 + a cos(k (theta - phase)) - star-shaped about c by construction, and not convex: a (k^2 + 1) > r0."""
    rng = np.random.RandomState(40_000 + seed)
    cx, cy = rng.uniform(0.42, 0.58, 2)
    r0 = rng.uniform(0.22, 0.28)
    a = rng.uniform(0.28, 0.36) * r0
    k = int(rng.randint(3, 6))
    phase = rng.uniform(0.0, 2.0 * np.pi)
    return float(cx), float(cy), float(r0), float(a), k, float(phase)


def star_mask(size: int = 64, seed: int = 0) -> np.ndarray:
    """bool (size, size), True = object, on the linspace(0, 1) grid of the prior datasets (x along the columns, y along the rows)."""
    cx, cy, r0, a, k, phase = star_shape(seed)
    lin = np.linspace(0.0, 1.0, size)
    yy, xx = np.meshgrid(lin, lin, indexing="ij")
    rad, theta = np.hypot(xx - cx, yy - cy), np.arctan2(yy - cy, xx - cx)
    return rad <= r0 + a * np.cos(k * (theta - phase))


def star_unaries(size: int = 64, seed: int = 0) -> torch.Tensor:
    """(size, size) float32 unaries of the seeded non-convex star, fg (object) = 0, bg = 1."""
    return torch.from_numpy(1.0 - star_mask(size, seed).astype(np.float32))


from .prior_dataset import PriorDataset, prior  # noqa: E402


class SyntheticPriorDataset(PriorDataset):
    """The synthetic inputs in the item format of the reference's prior datasets (AwesomeDataset.__getitem__,
    awesome/dataset/awesome_dataset.py:291-294, wrapped by `@prior()`):

        ((index, prior_state), ((image, features, xy_clean), target))

    `image` (1, S, S) holds segmentation LOGITS whose sigmoid, inverted, is the unaries of the synthetic item (so
    WrapperModule(ForwardModule(), prior, use_segmentation_output_inversion=...) reproduces them like a trained backbone would);
    `features` is an empty placeholder, `xy_clean` the (2, S, S) linspace grid of Transformator.get_positional_matrices, `target`
    (1, S, S) the clean mask in the unaries' convention (object = 0, background = 1: what the inverted segmentation output is
    trained against).  `kind`: 'blob' | 'noisy_blob' | 'disc' (see SyntheticUnariesDataset).  `features='xy'`: the features are
    the (2, S, S) grid as well (the spatial features a CNNNet with 'rgbxy' input reads)."""

    returns_index = False
    training_batch_size = 1

    def __init__(self, n_images: int = 1, size: int = 256, kind: str = "blob", seed0: int = 0, prior_model_type=None,
                 prior_model_args=None, features: str = "none", **kwargs):
        super().__init__(prior_model_type=prior_model_type, prior_model_args=prior_model_args)
        if features not in ("none", "xy"):
            raise ValueError(f"features must be 'none' or 'xy' but is {features!r}")
        self.kind = kind
        self.features = features
        if kind == "sequence":
            masks = dumbbell_sequence_masks(int(size), int(n_images), int(seed0))
            frames = [torch.from_numpy(1.0 - m.astype(np.float32)) for m in masks]
            self._inner = SyntheticUnariesDataset(n_images=n_images, size=size, kind="blob", seed0=seed0)
            self._inner.unaries = lambda i: frames[int(i)]
            self._inner.ground_truth = lambda i: frames[int(i)]
        else:
            self._inner = SyntheticUnariesDataset(n_images=n_images, size=size, kind=kind, seed0=seed0)
        self.size = int(size)
        xs = torch.linspace(0, 1, self.size)
        self._xy = torch.stack([xs[None, :].expand(self.size, self.size), xs[:, None].expand(self.size, self.size)], 0).contiguous()

    def __len__(self) -> int:
        return len(self._inner)

    def unaries(self, i: int) -> torch.Tensor:
        return self._inner.unaries(i)

    def ground_truth(self, i: int) -> torch.Tensor:
        return self._inner.ground_truth(i)

    def ground_truth_batch(self, indices) -> torch.Tensor:
        return self._inner.ground_truth_batch(indices)

    # ---- the rest of the reference's dataset contract -----------------------------------------------------------
    def decode_encoding(self, output: torch.Tensor) -> torch.Tensor:
        """AwesomeDataset.decode_encoding (awesome/dataset/awesome_dataset.py:393-412), binary, 2-D: `>= 0.5`."""
        return (output >= 0.5).to(dtype=torch.float32)

    def split_indices(self):
        """(train, validation) indices (awesome_dataset.py:169-171): every synthetic image is a training image - the per-image
        fits have nothing to validate on."""
        return np.arange(len(self)), np.zeros((0,), dtype=np.int64)

    def get_config(self):
        """base_dataset.py:51-60: the constructor arguments."""
        return dict(n_images=len(self), size=self.size, kind=self.kind, returns_index=self.returns_index,
                    training_batch_size=self.training_batch_size)

    @prior()
    def __getitem__(self, i: int):
        un = self._inner.unaries(int(i)).clamp(1e-6, 1 - 1e-6)
        fg_prob = 1.0 - un                                   # probability of "object" = what sigmoid(seg logits) is
        image = torch.log(fg_prob / (1.0 - fg_prob))[None]   # logits; sigmoid(image) = fg_prob
        target = (self._inner.ground_truth(int(i)) > 0.5).float()[None]
        xy = self._xy
        if self.kind == "sequence":
            t = float(i) / float(max(len(self) - 1, 1))
            xy = torch.cat([xy, torch.full((1, self.size, self.size), t)], 0)
        feat = xy.clone() if self.features == "xy" else torch.zeros(1, 1, 1)
        return (image, feat, xy), target


class SyntheticPixelDataset(SyntheticPriorDataset):
    """The synthetic inputs for the pixel mode of the convexity configs (`dataset_args.dimension: 2d`, AwesomeDataset
    .get_dimension_based_data, awesome/dataset/awesome_dataset.py:198-217, 296-326).  Indexing gives SyntheticPriorDataset's image
    items (what the per-image prior fits read); `pixel_item(i)` is the training item of the joint epochs:

        ((rgb rows (n, 3), feature rows (n, 2), clean-xy rows (n, 2)), target (n_scr, 1))

    in the reference's order: the scribbled pixels first (row-major, as a boolean mask selects them), then ceil(n_scr (1 / p - 1))
    distinct pixels drawn with the seed `split_seed` (also row-major), p = scribble_percentage.  The image is synthetic RGB: one
    colour per class plus seeded noise; the scribbles are `n_scribble` seeded pixels labelled with the clean mask in the unaries'
    convention (object = 0, background = 1); the features are the pixel's coordinates (the 'rgbxy' input of the FCNet configs)."""

    dimension = "2d"

    def __init__(self, n_images: int = 1, size: int = 256, kind: str = "blob", seed0: int = 0, prior_model_type=None,
                 prior_model_args=None, scribble_percentage: float = 0.8, n_scribble: int = 0, split_seed: int = 42,
                 dimension: str = "2d", **kwargs):
        kwargs.pop("features", None)
        super().__init__(n_images=n_images, size=size, kind=kind, seed0=seed0, prior_model_type=prior_model_type,
                         prior_model_args=prior_model_args, features="xy", **kwargs)
        if dimension != "2d":
            raise ValueError(f"SyntheticPixelDataset is the 2d (pixel) form of the dataset; dimension {dimension!r} is SyntheticPriorDataset")
        if not 0.0 < float(scribble_percentage) <= 1.0:
            raise ValueError("scribble_percentage must be in (0, 1]")
        self.scribble_percentage, self.split_seed = float(scribble_percentage), int(split_seed)
        n = int(n_scribble) if n_scribble else max(4, (self.size * self.size) // 8)
        n = min(n, self.size * self.size)
        # the losses recover the scribble count as floor(total * p): keep a count for which that round trip is exact
        while n > 1 and int((n + self._n_random(n)) * self.scribble_percentage // 1) != n:
            n -= 1
        self.n_scribble = n

    def _n_random(self, n_scr: int) -> int:
        if self.scribble_percentage >= 1.0:
            return 0
        return int(np.ceil(n_scr * (1.0 / self.scribble_percentage) - n_scr))

    def rgb(self, i: int) -> torch.Tensor:
        """(S * S, 3) float32 in [0, 1]."""
        rng = np.random.RandomState(20_000 + self._inner.seed0 + int(i))
        obj = (self._inner.ground_truth(int(i)) <= 0.5).numpy().reshape(-1, 1)
        colour = np.where(obj, np.array([[0.8, 0.3, 0.2]]), np.array([[0.2, 0.4, 0.7]]))
        return torch.from_numpy(np.clip(colour + rng.normal(scale=0.1, size=colour.shape), 0.0, 1.0).astype(np.float32))

    def pixel_rows(self, i: int):
        """Every pixel of image i as rows: (rgb (S*S, 3), features (S*S, 2), clean xy (S*S, 2)) - the evaluation input."""
        xy = self._xy.reshape(2, -1).t().contiguous()
        return self.rgb(i), xy.clone(), xy

    def pixel_item(self, i: int):
        rgb, feat, xy = self.pixel_rows(i)
        n_pix = rgb.shape[0]
        rng = np.random.RandomState(30_000 + self._inner.seed0 + int(i))
        scr = np.zeros(n_pix, dtype=bool)
        scr[rng.choice(n_pix, size=self.n_scribble, replace=False)] = True
        target = (self._inner.ground_truth(int(i)) > 0.5).float().reshape(-1)[torch.from_numpy(scr)][:, None]
        sel = [np.flatnonzero(scr)]
        n_rand = self._n_random(self.n_scribble)
        if n_rand > 0:
            if n_rand > n_pix:
                raise ValueError("Could not draw enough random pixels")
            rng = np.random.RandomState(self.split_seed)
            mask = np.zeros(n_pix, dtype=bool)
            for _ in range(1000):            # randint may draw a pixel twice: draw until enough distinct ones are marked
                need = n_rand - int(mask.sum())
                if need <= 0:
                    break
                mask[rng.randint(0, n_pix, size=need)] = True
            if int(mask.sum()) < n_rand:
                raise ValueError("Could not draw enough random pixels after 1000 iterations.")
            sel.append(np.flatnonzero(mask))
        idx = torch.from_numpy(np.concatenate(sel))
        return (rgb[idx], feat[idx], xy[idx]), target


class SyntheticUnariesDataset:
    """Minimal stand-in for the reference's prior datasets on the hot path: item i is `(grid_desc, unaries_i)` where
    unaries follow the reference convention (fg = 0).  `kind`: 'disc' (C1), 'blob' (C2/C3, seed = index + seed0),
    'noisy_blob' (C5: soft unaries from noisy synthetic logits) or 'star' (C8: a seeded non-convex star, star_shape)."""

    def __init__(self, n_images: int = 1, size: int = 256, kind: str = "blob", seed0: int = 0, **kwargs):
        self.n_images, self.size, self.kind, self.seed0 = int(n_images), int(size), kind, int(seed0)

    def __len__(self) -> int:
        return self.n_images

    def unaries(self, i: int) -> torch.Tensor:
        if self.kind == "disc":
            s = self.size
            return disc_unaries(s, s, s / 2, s / 2, 15.0 * s / 64.0)
        if self.kind == "blob":
            return convex_blob_unaries(self.size, self.seed0 + i)
        if self.kind == "noisy_blob":
            return noisy_blob_unaries(self.size, self.seed0 + i)
        if self.kind == "star":
            return star_unaries(self.size, self.seed0 + i)
        raise ValueError(f"unknown kind {self.kind}")

    def ground_truth(self, i: int) -> torch.Tensor:
        """Clean unaries (fg = 0) of item i - what a refinement is scored against."""
        if self.kind == "noisy_blob":
            return convex_blob_unaries(self.size, self.seed0 + i)
        return (self.unaries(i) > 0.5).float()

    def ground_truth_batch(self, indices) -> torch.Tensor:
        return torch.stack([self.ground_truth(int(i)).reshape(-1) for i in indices])

    def __getitem__(self, i: int):
        return (self.size, self.size), self.unaries(i)

    def batch(self, indices) -> torch.Tensor:
        return torch.stack([self.unaries(int(i)).reshape(-1) for i in indices])


def dumbbell_sequence_masks(size: int = 128, frames: int = 16, seed: int = 0) -> np.ndarray:
    """C4 '(x,y,t) sequence' (SURVEY.md §8d): an object of two discs joined by a thin bar, translating 2 px per frame; in
    every third frame the bar is missing (the object is only connected through time) - the case the path-connectedness
    prior over (x, y, t) exists for.  Returns bool (frames, size, size), True = object."""
    rng = np.random.RandomState(seed)
    s = size / 128.0
    cy, cx = rng.uniform(50.0, 78.0) * s, rng.uniform(40.0, 56.0) * s
    r, d, bar = 14.0 * s, 26.0 * s, max(1.0, 1.5 * s)
    ang = rng.uniform(-0.5, 0.5)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    out = np.zeros((frames, size, size), dtype=bool)
    for t in range(frames):
        ox, oy = cx + 2.0 * t * s, cy + 0.5 * t * s
        ax, ay = ox - d * np.cos(ang), oy - d * np.sin(ang)
        bx, by = ox + d * np.cos(ang), oy + d * np.sin(ang)
        m = ((xx - ax) ** 2 + (yy - ay) ** 2 <= r * r) | ((xx - bx) ** 2 + (yy - by) ** 2 <= r * r)
        if t % 3 != 2:
            # distance to the segment a-b
            px, py = xx - ax, yy - ay
            vx, vy = bx - ax, by - ay
            u = np.clip((px * vx + py * vy) / (vx * vx + vy * vy), 0.0, 1.0)
            m |= (px - u * vx) ** 2 + (py - u * vy) ** 2 <= bar * bar
        out[t] = m
    return out


class SyntheticSequenceDataset:
    """Item i = one (x, y, t) sequence for the spatio-temporal prior: `coords(i)` (3, T*H*W) = linspace(0,1) x linspace(0,1) x
    t/t_max (awesome/dataset/transformator.py:25-61) and `unaries(i)` (T*H*W,) with fg = 0."""

    def __init__(self, n_sequences: int = 1, size: int = 128, frames: int = 16, seed0: int = 0, **kwargs):
        self.n_images, self.size, self.frames, self.seed0 = int(n_sequences), int(size), int(frames), int(seed0)

    def __len__(self) -> int:
        return self.n_images

    def coords(self) -> torch.Tensor:
        s, t = self.size, self.frames
        lin = torch.linspace(0, 1, s)
        ts = torch.arange(t).float() / float(max(t - 1, 1))
        tt, yy, xx = torch.meshgrid(ts, lin, lin, indexing="ij")
        return torch.stack([xx.reshape(-1), yy.reshape(-1), tt.reshape(-1)], 0)

    def unaries(self, i: int) -> torch.Tensor:
        m = dumbbell_sequence_masks(self.size, self.frames, self.seed0 + i)
        return torch.from_numpy(1.0 - m.astype(np.float32)).reshape(-1)

    def batch(self, indices) -> torch.Tensor:
        return torch.stack([self.unaries(int(i)) for i in indices])
