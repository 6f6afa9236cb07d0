"""Plain torch references of the optional losses, the evaluation metrics, the streaming moments and Adam, in the dtype and on the device of
their arguments (the tests call them in float64, and in float32 for "the reference's own fp32 deviation"), and the bound the metric tests
share.  Where oracle/pulpo_oracle.py is device-generic the reference is the oracle's expression; the Jacobian determinant and KL_nondiagonal
build their index and degree tensors on the argument's device.  tests/test_host_metrics_ref.py pins all of them to the oracle and to the
goldens made with the reference project (tests/golden/metrics.npz, evalmetrics.npz); tests/test_gpu_pyramid_metrics.py holds the HIP
kernels to them."""
import torch

import pyramid_ref as R
from oracle import pulpo_oracle as O

l2_loss = O.l2_loss                     # spatial sum of squared differences, mean over batch and channels
soft_dice = O.soft_dice                 # mean_(b,c) (1 - (2<t,i> + 1e-6) / (|t|^2 + |i|^2 + 1e-6)) * voxels / dice_factor
rmse = O.rmse                           # sqrt(mean((a - b)^2)); the target broadcasts
dsc = O.dsc
mc_std_map = O.mc_std_map               # (N, C, ...) samples -> mean over C of the unbiased std over N, optionally of stack * scale


def jacobian_det(df, normalize: bool = True):
    """determinant of I + grad u, central differences on a replicate-padded field (src/losses.py:153-199): (B,3,D,H,W) -> (B,D,H,W) and
    (B,2,H,W) -> (B,H,W).  The reference's quirks as in O.jacobian_det: channel i scaled by 2 / S_i when normalising, then the channels
    flipped and flipped channel c scaled by (S_c - 2) / 2"""
    S = tuple(df.shape[2:])
    nd = len(S)
    assert df.shape[1] == nd and nd in (2, 3), tuple(df.shape)
    u = torch.stack([df[:, i] * 2 / S[i] for i in range(nd)], dim=1) if normalize else df
    uf = u.flip(1) * torch.tensor([(s - 2) / 2 for s in S], dtype=df.dtype, device=df.device).view(1, nd, *([1] * nd))
    J = [[None] * nd for _ in range(nd)]
    for a in range(nd):                                  # derivative axis
        idx = torch.arange(S[a], device=df.device)
        g = 0.5 * (uf.index_select(2 + a, (idx + 1).clamp(max=S[a] - 1)) - uf.index_select(2 + a, (idx - 1).clamp(min=0)))
        for c in range(nd):
            J[a][c] = g[:, c] + (1.0 if a == c else 0.0)
    if nd == 2:
        return J[0][0] * J[1][1] - J[1][0] * J[0][1]
    return (J[0][0] * (J[1][1] * J[2][2] - J[2][1] * J[1][2]) - J[0][1] * (J[1][0] * J[2][2] - J[2][0] * J[1][2])
            + J[0][2] * (J[1][0] * J[2][1] - J[2][0] * J[1][1]))


def jacobian_det_2d(df, normalize: bool = True):
    """the reference's 2-D determinant (src/losses.py:153-171) of a (B,2,H,W) field in its dtype"""
    assert df.dim() == 4
    return jacobian_det(df, normalize)


def jdet_std(df, lamb: float = 0.0, normalize: bool = True):
    """lamb * unbiased std of the Jacobian determinant (src/losses.py:202-204)"""
    return lamb * jacobian_det(df, normalize).std()


def degree(S, dtype, device):
    """number of in-volume voxels of the 3^ndims neighbourhood, minus one: the D of KL_nondiagonal"""
    d = None
    for a, s in enumerate(S):
        i = torch.arange(s, device=device)
        n = ((i + 1).clamp(max=s - 1) - (i - 1).clamp(min=0) + 1).to(dtype).view([-1 if k == a else 1 for k in range(len(S))])
        d = n if d is None else d * n
    return d - 1


def kl_nondiagonal(mu, sigma, prior_lambda: float = 20.0):
    """KL_nondiagonal.loss (src/losses.py:8-44), O.kl_nondiagonal's expression: mean(lambda D sigma^2 - log sigma^2) plus lambda / 2 times
    the mean squared forward difference of mu per axis (averaged over the axes, halved), times ndims / 2 * voxels"""
    S = tuple(mu.shape[2:])
    nd = len(S)
    s2 = sigma ** 2
    sigma_term = prior_lambda * degree(S, mu.dtype, mu.device) * s2 - torch.log(s2)
    sm = 0
    for a in range(nd):
        d = mu.narrow(2 + a, 1, S[a] - 1) - mu.narrow(2 + a, 0, S[a] - 1)
        sm = sm + (d * d).mean()
    V = 1
    for s in S:
        V *= s
    return (sigma_term.mean() + (prior_lambda / 2) * (0.5 * sm / nd)) * nd * 0.5 * float(V)


def percent_leq0(x):
    """100 * count(x <= 0) / numel, the count exact (an integer)"""
    return 100.0 * int((x <= 0).sum()) / x.numel()


def warp_landmarks(lm, df):
    """Evaluate.warp_landmarks (evaluate.py:410-423): lm.long() - df[:, :, lm...] transposed, (1, n, ndims) and (samples, ndims, ...) ->
    (samples, n, ndims); negative indices wrap and an index outside the field raises IndexError, as tensor indexing does"""
    i = lm.long()
    return i - df[(slice(None), slice(None)) + tuple(i[0, :, c] for c in range(i.shape[2]))].transpose(-2, -1)


def adam_ref(p, g, m, v, lr: float, step: int, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, gscale: float = 1.0):
    """one torch.optim.Adam update (no weight decay, no amsgrad) of (p, m, v) with the gradient g * gscale, bias corrections 1 - beta^step;
    returns the new (p, m, v) in the dtype of the arguments"""
    gr = g * gscale
    m = beta1 * m + (1 - beta1) * gr
    v = beta2 * v + (1 - beta2) * gr * gr
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    return p - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps), m, v


# ------------------------------------------------------------------------------------------------ the bound
def spread(ref32, ref64) -> float:
    """max |fp32 evaluation - float64 evaluation| of a reference: its own fp32 deviation"""
    return R.ratio(ref32, ref64, 1.0)


def bound(ref32, ref64, floor_rel: float, k: float = 4.0) -> float:
    """the rule of the metric tests: max(k x the reference's own fp32 deviation, floor_rel x max|ref|), an absolute tolerance"""
    return max(k * spread(ref32, ref64), floor_rel * float(ref64.detach().abs().max()))


def rel(a, b) -> float:
    return abs(float(a) - float(b)) / abs(float(b))
