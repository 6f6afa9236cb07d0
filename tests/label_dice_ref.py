"""The Dice term of the training step from label maps, by its definition in plain torch (any dtype, any device): one_hot of the moving
label map -> the reference's warp (O.warp through pyramid_ref.warp_ref; for slices the same normalisation with a 2-D grid_sample) ->
against the resized one-hot target (pyramid_ref.resize_ref) -> metrics_ref.soft_dice.  Autograd gives the gradient with respect to the
field.  tests/test_host_label_dice.py pins the definition's gradient with gradcheck; tests/test_gpu_label_dice.py holds
ops.label_dice_loss and ops.labels_soft_map to it.  Also the construction of the test fields: displacements made from chosen sample
coordinates, so that no sample sits where the trilinear gradient jumps."""
import torch
import torch.nn.functional as F

import metrics_ref as M
import pyramid_ref as R


def one_hot(labels, C: int, dtype):
    """(B, 1, ...) integer labels -> (B, C, ...) in dtype; a label outside [0, C) belongs to no class"""
    lab = labels.long()
    cls = torch.arange(C, device=lab.device).view(1, C, *([1] * (lab.dim() - 2)))
    return (lab == cls).to(dtype)


def warp(df, img):
    """SpatialTransformer on df's device and dtype: (B,3,D,H,W) fields through pyramid_ref.warp_ref, (B,2,H,W) fields by the same rule -
    positions normalised by (S - 1), sampled bilinearly with border padding and align_corners=False"""
    if df.dim() == 5:
        return R.warp_ref(df, img)
    H, W = df.shape[2:]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=df.dtype, device=df.device), torch.arange(W, dtype=df.dtype, device=df.device), indexing="ij")
    ny = 2 * ((ys + df[:, 0]) / (H - 1) - 0.5)
    nx = 2 * ((xs + df[:, 1]) / (W - 1) - 0.5)
    return F.grid_sample(img, torch.stack([nx, ny], dim=-1), mode="bilinear", padding_mode="border", align_corners=False)


def resize(x, size):
    """F.interpolate(x, size, tri/bilinear, align_corners=False) in x's dtype (pyramid_ref.resize_ref; slices as depth-1 volumes)"""
    if x.dim() == 4:
        return R.resize_ref(x.unsqueeze(2), (1,) + tuple(size)).squeeze(2)
    return R.resize_ref(x, tuple(size))


def maps(df, labels, C: int, target):
    """(p, t): the warped one-hot moving map and the resized one-hot target on df's grid, in df's dtype"""
    p = warp(df, one_hot(labels, C, df.dtype))
    t = resize(one_hot(target, C, df.dtype), df.shape[2:])
    return p, t


def label_dice_loss(df, labels, C: int, target, dice_factor=1):
    p, t = maps(df, labels, C, target)
    return M.soft_dice(p, t, dice_factor)


def dice_per_class(df, labels, C: int, target):
    """(B, C): (2 sum(p t) + 1e-6) / (sum(t^2) + sum(p^2) + 1e-6)"""
    p, t = maps(df, labels, C, target)
    return (2.0 * (t * p).flatten(2).sum(2) + 1e-6) / ((t ** 2).flatten(2).sum(2) + (p ** 2).flatten(2).sum(2) + 1e-6)


# ------------------------------------------------------------------------------------------------ fields from chosen sample coordinates
def coords_of(df, img_size):
    """(B, nd, grid): the unclamped sample coordinate in image voxels per axis, ((2 ((p + d) / (Sg - 1) - 0.5) + 1) Si - 1) / 2, evaluated
    operation by operation in df's dtype as the kernels' sample_coord does"""
    nd = df.shape[1]
    out = []
    for a in range(nd):
        Sg, Si = df.shape[2 + a], img_size[a]
        pos = torch.arange(Sg, dtype=df.dtype, device=df.device).view([-1 if k == a else 1 for k in range(nd)])
        t = (pos + df[:, a]) / (Sg - 1)
        t = 2 * (t - 0.5)
        out.append(((t + 1) * Si - 1) / 2)
    return torch.stack(out, dim=1)


def field_from_coords(coords, img_size):
    """the inverse of coords_of, in float64: the displacement d = (c + 0.5) (Sg - 1) / Si - p that puts voxel p's sample at coordinate c"""
    nd = coords.shape[1]
    c = coords.double()
    out = []
    for a in range(nd):
        Sg, Si = c.shape[2 + a], img_size[a]
        pos = torch.arange(Sg, dtype=torch.float64, device=c.device).view([-1 if k == a else 1 for k in range(nd)])
        out.append((c[:, a] + 0.5) * (Sg - 1) / Si - pos)
    return torch.stack(out, dim=1)


def make_field(B, grid, img_size, gen, slab: bool = True):
    """(df fp32 (B, nd, grid), clamped bool (B, nd, grid)).  Every sample coordinate is an integer in [0, Si - 2] plus a fraction in
    [0.05, 0.95]: no sample within 0.05 of where the trilinear gradient jumps.  slab: in the first plane of the grid's first axis the
    voxels take turns, one axis each, at 1.3 voxels below the first or above the last sample of that axis (clamped there)."""
    nd = len(grid)
    base = torch.stack([torch.randint(0, max(img_size[a] - 1, 1), (B, *grid), generator=gen).double() for a in range(nd)], dim=1)
    frac = 0.05 + 0.9 * torch.rand((B, nd, *grid), generator=gen, dtype=torch.float64)
    coords = base + frac
    clamped = torch.zeros((B, nd, *grid), dtype=torch.bool)
    if slab:
        n = coords[0, 0, 0].numel()
        k = torch.arange(n).view(coords[0, 0, 0].shape)
        for a in range(nd):
            for side in (0, 1):
                sel = ((k % nd) == a) & (((k // nd) % 2) == side)
                coords[:, a, 0][:, sel] = -1.3 if side == 0 else (img_size[a] - 1) + 1.3
                clamped[:, a, 0][:, sel] = True
    return field_from_coords(coords, img_size).float(), clamped


def assert_floor_agrees(df, img_size, clamped):
    """the input condition of the gradient comparison: at every voxel and axis that the construction did not clamp, the fp32 and the
    float64 evaluation of the sample coordinate fall into the same cell, strictly inside the map"""
    c32, c64 = coords_of(df, img_size), coords_of(df.double(), img_size)
    free = ~clamped
    assert bool((c32.floor().double() == c64.floor())[free].all()), "fp32 and float64 disagree about a sample's cell"
    for a in range(df.shape[1]):
        ca, fa = c64[:, a], free[:, a]
        assert bool(((ca > 0) & (ca < img_size[a] - 1))[fa].all()), "an unclamped sample lies outside the map"
        assert bool(((ca < 0) | (ca > img_size[a] - 1))[~fa].all()), "a sample meant to be clamped is not"


def make_labels(B, shape, C: int, dtype, gen, target: bool):
    """(B, 1, shape) labels in 2-voxel blocks (equal and different neighbours).  Class C - 1 is in no map; class C - 2 only in a target;
    the batch elements use different label sets (element b draws from the classes below C - 2 - b, at least 2)."""
    half = [(s + 1) // 2 for s in shape]
    out = []
    for b in range(B):
        hi = max(C - 2 - b, 2)
        lab = torch.randint(0, hi, (1, 1, *half), generator=gen)
        for a, s in enumerate(shape):
            lab = lab.repeat_interleave(2, dim=2 + a).narrow(2 + a, 0, s)
        if target:
            lab = lab.contiguous().clone()
            lab.view(-1)[1::7] = C - 2
        out.append(lab)
    return torch.cat(out).to(dtype)
