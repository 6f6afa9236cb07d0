"""On-device training augmentation: random affine + cubic B-spline elastic maps and an intensity transform, applied to
a batch that already lives on the GPU by one fused kernel per image (`ops.augment`), which pulls the image, its mask and its label map through
one evaluation of the map and writes neither a sampling grid nor a displacement field.

    aug = Augmenter(size=(160, 160, 160), seed=0, rotate_deg=10, scale=0.1, translate_vox=4, elastic_spacing=16, elastic_std_vox=1.5,
                    gamma=0.3, noise_std=0.03, bias_std=0.2)
    for batch in AugmentedLoader(DevicePrefetcher(train_loader, device), aug):
        stepper.step(batch)

Every random number comes from the augmenter's own CPU torch.Generator, so a seed gives the same parameters on any device; they travel to
the GPU through pinned memory with non-blocking copies, and nothing is ever read back (no .item(), no synchronisation) - the noise is made on
the device by a counter-based generator from a drawn seed.  The reference's datasets (src/data) hand out raw pairs: it has no counterpart.
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, Iterator, Optional, Sequence

import torch

from . import ops


def _per_axis(v, nd: int, name: str):
    if isinstance(v, (int, float)):
        return [float(v)] * nd
    v = [float(a) for a in v]
    if len(v) != nd:
        raise ValueError(f"Augmenter: {name} is one number or {nd} numbers, got {len(v)}")
    return v


def _eye(n: int):
    return [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]


def _matmul(A, B):
    return [[sum(a * B[k][j] for k, a in enumerate(row)) for j in range(len(B[0]))] for row in A]


class Augmenter:
    """Draws per-sample augmentation parameters and applies them with ops.augment.  `size`: the grid (D,H,W), or (H,W) for slices.  Ranges
    (a zero range switches the piece off; with every range zero the parameters are the identity and a batch passes through bit for bit):
      rotate_deg     angles uniform in [-r, r] degrees about each axis (one number or one per axis; slices: the single in-plane angle)
      scale          per-axis factors uniform in [1 - s, 1 + s]
      shear          the off-diagonal entries above the diagonal uniform in [-h, h]
      translate_vox  per-axis shifts uniform in [-t, t] voxels (one number or one per axis)
      flip_axes      spatial axes (0 = the first of `size`) mirrored with probability 1/2 each
      rigid          rotations, flips and shifts only: scale and shear are ignored and M M^T = I
      elastic_spacing, elastic_std_vox   control-lattice spacing s >= 2 (voxels) and the standard deviation of its N(0, std^2) entries (voxels)
      gamma          the exponent exp(u), u uniform in [-g, g];  gain uniform in [1 - g, 1 + g];  offset uniform in [-o, o]
      noise_std      sigma uniform in [0, n];  bias_std: a log-bias lattice of bias_nodes^ndims N(0, std^2) nodes spanning the volume
      clip           clamp the image to [0, 1] at the end - whenever some intensity piece is drawn
      shared_spatial both images of a pair take the same spatial map (their intensity draws stay independent)
    M = R Sh diag(scale) F maps output voxels to input positions: p = c + M (v + e(v) - c) + t."""

    def __init__(self, size: Sequence[int], seed: int = 0, rotate_deg=0.0, scale: float = 0.0, shear: float = 0.0, translate_vox=0.0,
                 flip_axes: Sequence[int] = (), elastic_spacing: Optional[int] = None, elastic_std_vox: float = 0.0, gamma: float = 0.0,
                 gain: float = 0.0, offset: float = 0.0, noise_std: float = 0.0, bias_std: float = 0.0, bias_nodes: int = 4, clip: bool = True,
                 shared_spatial: bool = False, rigid: bool = False):
        self.size = tuple(int(s) for s in size)
        self.nd = len(self.size)
        if self.nd not in (2, 3) or min(self.size) < 1:
            raise ValueError(f"Augmenter: size (D,H,W) or (H,W) expected, got {size}")
        self.nrot = 3 if self.nd == 3 else 1
        self.rotate_deg = _per_axis(rotate_deg, self.nrot, "rotate_deg")
        self.translate_vox = _per_axis(translate_vox, self.nd, "translate_vox")
        self.scale, self.shear = float(scale), float(shear)
        self.flip_axes = tuple(int(a) for a in flip_axes)
        if any(a < 0 or a >= self.nd for a in self.flip_axes):
            raise ValueError(f"Augmenter: flip_axes are spatial axes 0..{self.nd - 1}, got {flip_axes}")
        self.elastic_std_vox = float(elastic_std_vox)
        self.elastic_spacing = None if elastic_spacing is None else int(elastic_spacing)
        if self.elastic_std_vox > 0 and (self.elastic_spacing is None or self.elastic_spacing < 2):
            raise ValueError("Augmenter: elastic_std_vox > 0 needs an elastic_spacing >= 2")
        self.gamma, self.gain, self.offset = float(gamma), float(gain), float(offset)
        self.noise_std, self.bias_std, self.bias_nodes = float(noise_std), float(bias_std), int(bias_nodes)
        if min(self.scale, self.shear, self.elastic_std_vox, self.gamma, self.gain, self.offset, self.noise_std, self.bias_std,
               *self.rotate_deg, *self.translate_vox) < 0 or self.scale >= 1 or self.gain >= 1 or self.bias_nodes < 1:
            raise ValueError("Augmenter: ranges are >= 0 (scale and gain below 1), bias_nodes >= 1")
        self.clip, self.shared_spatial, self.rigid = bool(clip), bool(shared_spatial), bool(rigid)
        self.seed = int(seed)
        self.generator = torch.Generator().manual_seed(self.seed)
        self.last_params = None

    # ------------------------------------------------------------------------------------------- drawing (CPU, float64)
    def _uniform(self, shape, lo, hi):
        return lo + (hi - lo) * torch.rand(shape, generator=self.generator, dtype=torch.float64)

    @property
    def elastic(self) -> bool:
        return self.elastic_std_vox > 0

    def _draw_spatial(self, B: int) -> Dict:
        nd = self.nd
        ang = torch.stack([self._uniform((B,), -r, r) for r in self.rotate_deg], dim=1) * (math.pi / 180.0)
        sc = self._uniform((B, nd), 1 - self.scale, 1 + self.scale)
        sh = self._uniform((B, nd * (nd - 1) // 2), -self.shear, self.shear)
        tr = torch.stack([self._uniform((B,), -t, t) for t in self.translate_vox], dim=1)
        flip = torch.rand((B, nd), generator=self.generator, dtype=torch.float64) < 0.5
        # the few matrix products per sample in plain Python floats (float64): a tenth of the host time of the same chain as tensor operations
        planes = [(1, 2), (0, 2), (0, 1)] if nd == 3 else [(0, 1)]      # rotation about axis k turns the plane of the other two
        upper = [(i, j) for i in range(nd) for j in range(i + 1, nd)]
        rows = []
        for a_b, s_b, h_b, t_b, f_b in zip(ang.tolist(), sc.tolist(), sh.tolist(), tr.tolist(), flip.tolist()):
            M = _eye(nd)
            for k, (i, j) in enumerate(planes):
                G = _eye(nd)
                c, s = math.cos(a_b[k]), math.sin(a_b[k])
                G[i][i], G[i][j], G[j][i], G[j][j] = c, -s, s, c
                M = _matmul(M, G)
            if not self.rigid:
                Sh = _eye(nd)
                for k, (i, j) in enumerate(upper):
                    Sh[i][j] = h_b[k]
                M = [[v * s_b[c] for c, v in enumerate(row)] for row in _matmul(M, Sh)]           # ... @ diag(scale)
            for a in self.flip_axes:
                if f_b[a]:
                    for row in M:
                        row[a] = -row[a]                                                          # ... @ F
            rows.append([row + [t_b[r]] for r, row in enumerate(M)])
        theta = torch.tensor(rows, dtype=torch.float64).float()
        phi = None
        if self.elastic:
            G = ops.bspline_lattice_size(self.size, self.elastic_spacing)
            phi = (self.elastic_std_vox * torch.randn((B, nd) + G, generator=self.generator, dtype=torch.float64)).float()
        return {"theta": theta, "phi": phi, "spacing": self.elastic_spacing if self.elastic else None}

    def _draw_intensity(self, B: int) -> Dict:
        out: Dict = {}
        if self.gamma > 0:
            out["gamma"] = torch.exp(self._uniform((B,), -self.gamma, self.gamma)).float()
        if self.gain > 0:
            out["gain"] = self._uniform((B,), 1 - self.gain, 1 + self.gain).float()
        if self.offset > 0:
            out["offset"] = self._uniform((B,), -self.offset, self.offset).float()
        if self.noise_std > 0:
            out["sigma"] = self._uniform((B,), 0.0, self.noise_std).float()
            out["seed"] = torch.randint(0, 2 ** 62, (1,), generator=self.generator, dtype=torch.int64)
        if self.bias_std > 0:
            out["bias"] = (self.bias_std * torch.randn((B,) + (self.bias_nodes,) * self.nd, generator=self.generator, dtype=torch.float64)).float()
        if out and self.clip:
            out["clip"] = True
        return out

    def draw(self, B: int) -> Dict:
        """the parameter set of one batch, as CPU tensors: {"x": map, "y": map}, a map = {"theta" (B,3,4) / (B,2,3), "phi" lattice or None,
        "spacing", "intensity": the dict of ops.augment}.  Under shared_spatial both maps hold the same theta and phi."""
        sx = self._draw_spatial(B)
        sy = sx if self.shared_spatial else self._draw_spatial(B)
        return {"x": dict(sx, intensity=self._draw_intensity(B)), "y": dict(sy, intensity=self._draw_intensity(B))}

    # ------------------------------------------------------------------------------------------- staging
    @staticmethod
    def to_device(params: Dict, device) -> Dict:
        """the parameter set on `device`: every tensor of it packed into one pinned buffer (two with the noise seeds), copied without blocking"""
        device = torch.device(device)
        floats, seeds = [], []

        def walk(d):
            for k, v in d.items():
                if isinstance(v, dict):
                    walk(v)
                elif torch.is_tensor(v) and not v.is_cuda:
                    (seeds if v.dtype == torch.int64 else floats).append(v)

        walk(params)
        moved = {}
        for group, dtype in ((floats, torch.float32), (seeds, torch.int64)):
            uniq = list({id(t): t for t in group}.values())                # (a shared map is staged once)
            if not uniq:
                continue
            host = torch.empty(sum(t.numel() for t in uniq), dtype=dtype, pin_memory=device.type == "cuda")
            torch.cat([t.reshape(-1) for t in uniq], out=host)
            dev = host.to(device, non_blocking=True)
            o = 0
            for t in uniq:
                moved[id(t)] = dev[o:o + t.numel()].view(t.shape)
                o += t.numel()

        def rebuild(d):
            return {k: rebuild(v) if isinstance(v, dict) else moved.get(id(v), v) if torch.is_tensor(v) else v for k, v in d.items()}

        return rebuild(params)

    # ------------------------------------------------------------------------------------------- applying
    def apply(self, params: Dict, img, mask=None, labels=None, intensity: bool = True):
        """ops.augment of one map (params["x"] or params["y"], CPU or device tensors) on an image with its mask and label map; returns the
        tuple of ops.augment.  intensity=False: the spatial part alone"""
        if any(torch.is_tensor(v) and v.device != img.device for v in (params["theta"], params["phi"])):
            params = self.to_device(params, img.device)
        return ops.augment(img, mask, labels, theta=params["theta"], phi=params["phi"], spacing=params["spacing"],
                           intensity=params["intensity"] if intensity else None)

    @staticmethod
    def _present(t) -> bool:
        return torch.is_tensor(t) and t.numel() > 0

    def _spatial_only(self, m: Dict, linear, nearest):
        """float tensors (trilinear) and integer tensors (nearest) through the map m, one launch per (float, integer) pair"""
        out_lin, out_near = [], []
        for i in range(max(len(linear), len(nearest))):
            a = linear[i] if i < len(linear) else None
            b = nearest[i] if i < len(nearest) else None
            res = list(ops.augment(None, a, b, theta=m["theta"], phi=m["phi"], spacing=m["spacing"]))
            if a is not None:
                out_lin.append(res.pop(0))
            if b is not None:
                out_near.append(res.pop(0))
        return out_lin, out_near

    def _one_side(self, m: Dict, img, seg, mask):
        """(img, seg, mask) through the map m: the image with intensity; float tensors trilinear, integer tensors nearest, in one launch where
        the kernel's three slots allow, the rest in a spatial-only launch with the same parameters"""
        linear, nearest, where = [], [], {}
        for name, t in (("seg", seg), ("mask", mask)):
            if not self._present(t):
                continue
            if t.dtype == torch.float32:
                where[name] = ("lin", len(linear))
                linear.append(t)
            elif t.dtype in (torch.uint8, torch.int32):
                where[name] = ("near", len(nearest))
                nearest.append(t)
            elif t.dtype == torch.bool:
                where[name] = ("near", len(nearest))
                nearest.append(t.to(torch.uint8))
            else:
                raise ValueError(f"Augmenter: {name} of dtype {t.dtype}: fp32 (one-hot maps, soft masks), uint8 / int32 (label maps) or bool expected")
        a = linear[0] if linear else None
        b = nearest[0] if nearest else None
        res = list(ops.augment(img, a, b, theta=m["theta"], phi=m["phi"], spacing=m["spacing"], intensity=m["intensity"]))
        out_img = res.pop(0)
        lin = [res.pop(0)] if a is not None else []
        near = [res.pop(0)] if b is not None else []
        more_lin, more_near = self._spatial_only(m, linear[1:], nearest[1:])
        got = {"lin": lin + more_lin, "near": near + more_near}
        outs = {}
        for name, t in (("seg", seg), ("mask", mask)):
            if name in where:
                kind, i = where[name]
                o = got[kind][i]
                outs[name] = o.to(torch.bool) if t.dtype == torch.bool else o
            else:
                outs[name] = t
        return out_img, outs["seg"], outs["mask"]

    def transport_landmarks(self, lm, theta):
        """landmarks (B,n,ndims) of an image, in voxels, carried to where the affine-augmented image shows them: the output voxel v samples the
        input at p = c + M (v - c) + t, so a point P of the input appears at v = c + M^-1 (P - c - t).  The inverse is formed in float64 on the
        host from the drawn (CPU) theta; the points stay on their device."""
        theta = theta.detach().cpu().double()
        if lm.dim() != 3 or lm.shape[2] != self.nd or lm.shape[0] != theta.shape[0]:
            raise ValueError(f"Augmenter: landmarks (B,n,{self.nd}) with the batch size of the images expected, got {tuple(lm.shape)}")
        Minv = torch.linalg.inv(theta[:, :, :self.nd])
        c = torch.tensor([(s - 1) / 2 for s in self.size], dtype=torch.float64)
        shift = c.unsqueeze(0) - torch.einsum("bij,bj->bi", Minv, c.unsqueeze(0) + theta[:, :, self.nd])      # v = M^-1 P + shift
        host = torch.cat([Minv.reshape(len(Minv), -1), shift], dim=1)
        if lm.is_cuda:
            host = host.pin_memory()
        dev = host.to(lm.device, non_blocking=True)
        Mi, sh = dev[:, :self.nd * self.nd].view(-1, self.nd, self.nd), dev[:, self.nd * self.nd:]
        out = torch.einsum("bij,bnj->bni", Mi, lm.double()) + sh.unsqueeze(1)
        return out.to(lm.dtype if lm.is_floating_point() else torch.float32)

    def __call__(self, batch):
        """the trainer's 8-tuple (x, y, seg_x, seg_y, lm1, lm2, mask1, mask2) -> the augmented 8-tuple.  x, seg_x and mask1 go through one
        spatial map, y, seg_y and mask2 through another (the same under shared_spatial); integer label maps take the nearest voxel, fp32
        one-hot maps and masks the trilinear route without intensity; empty placeholders pass through; landmarks follow an affine-only map
        by its inverse and are refused when the map has an elastic part.  The parameters used are kept in self.last_params (CPU tensors)."""
        x, y, seg_x, seg_y, lm1, lm2, mask1, mask2 = batch
        if self.elastic and (self._present(lm1) or self._present(lm2)):
            raise ValueError("Augmenter: landmarks cannot follow an elastic deformation (elastic landmark transport is not implemented); "
                             "set elastic_std_vox=0 or pass empty landmark placeholders")
        if tuple(x.shape[2:]) != self.size or tuple(y.shape[2:]) != self.size:
            raise ValueError(f"Augmenter: built for the grid {self.size}, got images {tuple(x.shape)} and {tuple(y.shape)}")
        params = self.draw(x.shape[0])
        self.last_params = params
        dev = self.to_device(params, x.device)
        x2, seg_x2, mask1_2 = self._one_side(dev["x"], x, seg_x, mask1)
        y2, seg_y2, mask2_2 = self._one_side(dev["y"], y, seg_y, mask2)
        lm1_2 = self.transport_landmarks(lm1, params["x"]["theta"]) if self._present(lm1) else lm1
        lm2_2 = self.transport_landmarks(lm2, params["y"]["theta"]) if self._present(lm2) else lm2
        return (x2, y2, seg_x2, seg_y2, lm1_2, lm2_2, mask1_2, mask2_2)


class AugmentedLoader:
    """iterate over `loader` (batches already on the device: put it after DevicePrefetcher) and yield every batch augmented.  For the
    training loader only: validation batches stay as they are."""

    def __init__(self, loader: Iterable, augmenter: Augmenter):
        self.loader, self.augmenter = loader, augmenter

    def __iter__(self) -> Iterator:
        for batch in self.loader:
            yield self.augmenter(batch)

    def __len__(self) -> int:
        return len(self.loader)
