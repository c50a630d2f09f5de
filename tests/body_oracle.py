"""A plain torch restatement of the SMPL-H forward (linear-blend skinning from its definition), dtype selectable; fp64 is the
yardstick the HIP body model is measured against.  Nothing here shares code with egoego_release_amd.body.

    v_shaped = v_template + shapedirs . betas            J = J_regressor . v_shaped
    R_j = Rodrigues(pose_j)                               offsets = posedirs . vec(R_1 - I, ..., R_51 - I)
    G_0 = [R_0 | J_0],  G_j = G_parent(j) [R_j | J_j - J_parent(j)]         A_j = G_j [I | -J_j]
    v = (sum_j w_vj A_j) (v_shaped + offsets) + trans     Jtr_j = t(G_j) + trans
"""
import numpy as np
import torch


def rodrigues(aa):
    """axis-angle [..., 3] -> rotation matrices [..., 3, 3]; exact at zero (the series of sin a / a and (1 - cos a) / a^2)."""
    x, y, z = aa.unbind(-1)
    a2 = x * x + y * y + z * z
    small = a2 < 1e-12
    a = torch.sqrt(torch.where(small, torch.ones_like(a2), a2))
    s = torch.where(small, 1 - a2 / 6, torch.sin(a) / a)
    c = torch.where(small, 0.5 - a2 / 24, 2 * torch.sin(a / 2) ** 2 / a ** 2)
    R = torch.stack([1 - c * (y * y + z * z), c * x * y - s * z, c * x * z + s * y,
                     c * x * y + s * z, 1 - c * (x * x + z * z), c * y * z - s * x,
                     c * x * z - s * y, c * y * z + s * x, 1 - c * (x * x + y * y)], -1)
    return R.reshape(aa.shape[:-1] + (3, 3))


def rodrigues_series(aa):
    """exp(K) by its Taylor series in long double, after halving K until |v| < 0.5 and squaring back: shares nothing with
    `rodrigues` (no sin, no cos, no switch point).  numpy [..., 3] -> long double [..., 3, 3]."""
    v = np.asarray(aa, np.longdouble)
    a = np.sqrt((v * v).sum(-1)).max() if v.size else 0.0
    halvings = max(0, int(np.ceil(np.log2(max(float(a), 0.5) / 0.5))))
    v = v / np.longdouble(2.0) ** halvings
    K = np.zeros(v.shape[:-1] + (3, 3), np.longdouble)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -v[..., 2], v[..., 1], v[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -v[..., 0], -v[..., 1], v[..., 0]
    R = np.zeros_like(K)
    R[..., 0, 0] = R[..., 1, 1] = R[..., 2, 2] = 1
    term = R.copy()
    for n in range(1, 40):
        term = np.einsum("...ab,...bc->...ac", term, K) / np.longdouble(n)
        R = R + term
    for _ in range(halvings):
        R = np.einsum("...ab,...bc->...ac", R, R)
    return R


def rodrigues_independent(aa):
    """An implementation of the rotation of an axis-angle vector that shares no line with `rodrigues`: scipy's
    Rotation.from_rotvec where scipy imports, else rodrigues_series.  numpy [..., 3] -> fp64 [..., 3, 3]."""
    aa = np.asarray(aa, np.float64)
    try:
        from scipy.spatial.transform import Rotation
    except ImportError:
        return rodrigues_series(aa).astype(np.float64)
    return Rotation.from_rotvec(aa.reshape(-1, 3)).as_matrix().reshape(aa.shape[:-1] + (3, 3))


def _split(x):
    """fp64 -> hi + lo in fp64: the two bf16 numbers a split-bf16 MFMA reads of the fp32 value (train_oracle._split)."""
    x32 = x.to(torch.float32)
    hi = x32.to(torch.bfloat16).to(torch.float32)
    lo = (x32 - hi).to(torch.bfloat16).to(torch.float32)
    return hi.to(torch.float64), lo.to(torch.float64)


def parents_of(model):
    p = np.asarray(model["kintree_table"]).astype(np.int64)[0].copy()
    p[0] = -1
    return p


def forward(model, pose, trans, betas, dtype=torch.float64, num_betas=16, split_offsets=False):
    """model: a dict of SMPL-H arrays; pose [N, 22 or 52, 3] axis-angle (missing hand joints at rest); trans [N, 3]; betas [N,
    num_betas] -> dict(v [N, V, 3], Jtr [N, 52, 3], offsets [N, V, 3], v_shaped [N, V, 3], J [N, 52, 3], A [N, 52, 3, 4]).
    `split_offsets` (fp64 only): the pose-offset contraction reads posedirs and the pose features as hi + lo bf16 and keeps the
    three products hi hi + lo hi + hi lo, summed exactly: the operand rounding of the kernel's GEMM and nothing else."""
    t = lambda a: torch.as_tensor(np.asarray(a).astype(np.float64) if not isinstance(a, torch.Tensor) else a).to(dtype)  # noqa: E731
    vt, sd, pd = t(model["v_template"]), t(model["shapedirs"])[:, :, :num_betas], t(model["posedirs"])
    jr, w = t(model["J_regressor"]), t(model["weights"])
    par = parents_of(model)
    pose, trans, betas = t(pose), t(trans), t(betas)
    N, nj = pose.shape[:2]
    if nj < 52:
        pose = torch.cat([pose, torch.zeros(N, 52 - nj, 3, dtype=dtype)], 1)
    v_shaped = vt[None] + torch.einsum("vcb,nb->nvc", sd, betas)
    J = torch.einsum("jv,nvc->njc", jr, v_shaped)
    R = rodrigues(pose)
    feat = (R[:, 1:] - torch.eye(3, dtype=dtype)).reshape(N, -1)
    if split_offsets:
        (ph, pl), (fh, fl) = _split(pd), _split(feat)
        offsets = torch.einsum("vck,nk->nvc", ph, fh) + torch.einsum("vck,nk->nvc", ph, fl) + torch.einsum("vck,nk->nvc", pl, fh)
    else:
        offsets = torch.einsum("vck,nk->nvc", pd, feat)
    Gr, Gt = [R[:, 0]], [J[:, 0]]
    for j in range(1, 52):
        p = int(par[j])
        Gr.append(Gr[p] @ R[:, j])
        Gt.append((Gr[p] @ (J[:, j] - J[:, p])[..., None])[..., 0] + Gt[p])
    Gr, Gt = torch.stack(Gr, 1), torch.stack(Gt, 1)
    At = Gt - (Gr @ J[..., None])[..., 0]
    A = torch.cat([Gr, At[..., None]], -1)  # [N, 52, 3, 4]
    T = torch.einsum("vj,njrc->nvrc", w, A)
    vp = v_shaped + offsets
    v = (T[..., :3] @ vp[..., None])[..., 0] + T[..., 3] + trans[:, None]
    return {"v": v, "Jtr": Gt + trans[:, None], "offsets": offsets, "v_shaped": v_shaped, "J": J, "A": A}
