"""Evaluation metrics of a training run without jetnet / energyflow: W1 of the jet mass (``w1m``), of the particle features
(``w1p``) and of five energy-flow polynomials (``w1efp``), coverage and MMD (``cov_mmd``), and the Frechet and kernel physics
distances (``fpd``, ``kpd``), as the reference's ``evaluate`` (train.py:543-606) appends them to its ``losses`` dict after every
epoch.

The names follow ``jetnet.utils`` / ``jetnet.evaluation`` so a caller can swap those modules for this one.  Jets are
``[n, N, >=3]`` un-normalised ``(eta_rel, phi_rel, pt_rel[, mask])`` with ``pt_rel = 0`` on padding particles (what
``gen.generate_jets`` returns).  The per-jet observables run on the GPU through ``mpg_jet_obs`` (fp32) for CUDA tensors,
and through a torch fp64 statement of the same formulas for CPU tensors and numpy arrays; the W1 distances are computed
in fp64 on the inputs' device.

The sampling semantics of ``w1m`` / ``w1p`` / ``w1efp`` (per batch ``rng.choice(len(real), k)`` then
``rng.choice(len(gen), k)``, with replacement; mean and population std over batches; ``exclude_zeros`` drops particles
whose feature norm is 0) are restated from memory of jetnet 0.2; jetnet is not available to check them against.  The same
holds for jetnet's EFP normalisation: ``normed=True`` (z_i = pT_i / sum pT) is energyflow's documented default, not a
checked property of ``jetnet.utils.efps``.

EFP columns (``efps``), hadronic measure with beta = 1 (theta_ij = sqrt(d_eta^2 + d_phi^2)), sums over all index tuples,
w = Theta z, u = (Theta o Theta) z, M = Theta diag(z) Theta -- the five connected multigraphs with 4 vertices and 4 edges
(energyflow's ``("n==", 4), ("d==", 4), ("p==", 1)`` set), in this project's order:

    0  a=b-c-d (end edge doubled)     sum_{b,c} z_b u_b theta_bc z_c w_c
    1  a-b=c-d (middle edge doubled)  sum_{b,c} z_b w_b theta_bc^2 z_c w_c
    2  3-star, one edge doubled       sum_c z_c u_c w_c^2
    3  triangle + pendant             sum_{a,c} z_a z_c w_c theta_ac M_ac
    4  4-cycle                        sum_{a,c} z_a z_c M_ac^2

Coverage and MMD (``cov_mmd``) come from the exact pairwise energy mover's distances of ``emds``: energyflow's ``emd`` with
``beta = 1``, ``norm = False``, no phi wrap, ``R = 1`` -- the transportation problem between the particles of positive pT of two
jets with cost theta_ij / R, the lighter jet completed by one slack particle of weight |sum pT_A - sum pT_B| at cost exactly 1
(``include/mpgan_amd.h`` has the statement in full).  Per batch ``i_real = rng.choice(len(real), k)`` then
``i_gen = rng.choice(len(gen), k)``, ``D[g, r] = EMD(gen[i_gen[g]], real[i_real[r]])``, ``mmd = mean_r min_g D[g, r]``,
``cov = |unique_g argmin_r D[g, r]| / k`` (argmin = first index of the minimum); the means over ``num_batches`` batches are
returned as ``(coverage, mmd)``.  Like the W1 sampling semantics above, the EMD conventions and the cov / mmd definition are
restated from memory of energyflow, jetnet 0.2 and the MPGAN paper; neither library is available to check them against (the
solver itself is checked against a linear-programming statement of the definition).  CUDA tensors run ``mpg_jet_emd`` (one
launch per distance matrix, fp32); CPU tensors and numpy arrays run the same solver in fp64 on up to 16 host threads.

FPD and KPD (``fpd``, ``kpd``; the reference picks its best epoch by ``fpd value + error``, train.py:794-809) are computed from
the 36 EFPs of degree <= 4, ``efps(jets, efpset_args=[("d<=", 4)])``.  The set is a definition, not a convention of energyflow:
every loopless multigraph with at most 4 edges and no isolated vertex, up to isomorphism, the graph of one vertex included --
1, 1, 3, 8, 23 graphs of degree 0 .. 4 (``EFP_D4_GRAPHS``; tests enumerate them from the definition).  21 of them are connected:
``mpg_jet_efps_d4`` (one launch, fp32; closed forms over row sums of powers of Theta and over M, table in
``include/mpgan_amd.h``) computes those for CUDA tensors, an fp64 torch statement of the same forms for CPU tensors and numpy
arrays; the other 15 are disjoint unions, whose EFPs are products of the connected ones' (``EFP_D4_FACTORS``), formed in fp64.
The column order is this project's; both metrics and the per-column normalisation they apply first are invariant under
permutations of the columns, so energyflow's order is not needed.  The sampling and extrapolation procedure of ``fpd`` and
``kpd`` is restated from memory of jetnet (their docstrings), like the W1 sampling semantics above.

FPND (jetnet's pretrained ParticleNet) is not provided.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib

NUM_EFPS = 5
MAX_PARTICLES = 160          # MPG_JET_OBS_MAX_N of include/mpgan_amd.h
_FLAG_EFP, _FLAG_NORMED = 1, 2
_CPU_CHUNK = 1 << 22         # fp64 pair elements per chunk of the CPU path (jets x N x N)


def _as_tensor(x):
    return (torch.from_numpy(np.ascontiguousarray(x)), True) if isinstance(x, np.ndarray) else (x, False)


def _out(t, numpy_in):
    return t.cpu().numpy() if numpy_in else t


# ------------------------------------------------------------------------------------- per-jet observables
def _obs_cuda(jets: torch.Tensor, with_efps: bool, normed: bool):
    n, N = jets.shape[0], jets.shape[1]
    if jets.dtype != torch.float32 or jets.stride(2) != 1:
        jets = jets.float().contiguous()
    kin = torch.empty((n, 4), device=jets.device, dtype=torch.float32)
    efp = torch.empty((n, NUM_EFPS), device=jets.device, dtype=torch.float32) if with_efps else None
    if n == 0:
        return kin, efp
    flags = (_FLAG_EFP if with_efps else 0) | (_FLAG_NORMED if normed else 0)
    with torch.cuda.device(jets.device):
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().mpg_jet_obs(jets.data_ptr(), jets.stride(0), jets.stride(1), n, N, flags, kin.data_ptr(),
                                          None if efp is None else efp.data_ptr(), stream), "mpg_jet_obs")
    return kin, efp


def _obs_cpu(jets: torch.Tensor, with_efps: bool, normed: bool):
    """fp64 statement of mpg_jet_obs, chunked over jets (the pair tensors are jets x N x N)."""
    x = jets[..., :3].double()
    n, N = x.shape[0], x.shape[1]
    kin = torch.empty((n, 4), dtype=torch.float64)
    efp = torch.empty((n, NUM_EFPS), dtype=torch.float64) if with_efps else None
    step = max(1, _CPU_CHUNK // max(1, N * N))
    for s in range(0, n, step):
        eta, phi, pt = x[s:s + step].unbind(-1)
        px, py, pz = (pt * phi.cos()).sum(1), (pt * phi.sin()).sum(1), (pt * eta.sinh()).sum(1)
        jpt = torch.hypot(px, py)
        deta = eta[:, :, None] - eta[:, None, :]
        dphi = phi[:, :, None] - phi[:, None, :]
        # cosh(d_eta) - cos(d_phi) = 2 sinh^2(d_eta / 2) + 2 sin^2(d_phi / 2)
        pair = 2 * ((0.5 * deta).sinh() ** 2 + (0.5 * dphi).sin() ** 2)
        m2 = torch.einsum("bi,bij,bj->b", pt, pair, pt)
        kin[s:s + step, 0] = jpt
        kin[s:s + step, 1] = torch.where(jpt > 0, torch.asinh(pz / torch.where(jpt > 0, jpt, 1.0)), 0.0)
        kin[s:s + step, 2] = torch.atan2(py, px)
        kin[s:s + step, 3] = m2.clamp(min=0).sqrt()
        if with_efps:
            if normed:
                spt = pt.sum(1, keepdim=True)
                z = pt / torch.where(spt != 0, spt, 1.0)
            else:
                z = pt
            th = (deta ** 2 + dphi ** 2).sqrt()
            w = torch.einsum("bij,bj->bi", th, z)
            u = torch.einsum("bij,bj->bi", th * th, z)
            M = torch.einsum("bij,bj,bjk->bik", th, z, th)
            zw = z * w
            efp[s:s + step, 0] = torch.einsum("bi,bij,bj->b", z * u, th, zw)
            efp[s:s + step, 1] = torch.einsum("bi,bij,bj->b", zw, th * th, zw)
            efp[s:s + step, 2] = (z * u * w * w).sum(1)
            efp[s:s + step, 3] = torch.einsum("bi,bij,bj->b", z, th * M, zw)
            efp[s:s + step, 4] = torch.einsum("bi,bij,bj->b", z, M * M, z)
    return kin, efp


def _observables(jets, with_efps: bool, normed: bool = True):
    """(kin [n, 4] = (pt, eta, phi, mass), efp [n, 5] or None) on the jets' device; numpy in, numpy out."""
    t, numpy_in = _as_tensor(jets)
    if t.dim() != 3 or t.shape[2] < 3:
        raise ValueError(f"expected jets [n, N, >=3] = (eta_rel, phi_rel, pt_rel, ...), got {tuple(t.shape)}")
    if t.is_cuda:
        if not 1 <= t.shape[1] <= MAX_PARTICLES:
            raise ValueError(f"mpg_jet_obs takes 1 <= N <= {MAX_PARTICLES} particles per jet (got {t.shape[1]})")
        kin, efp = _obs_cuda(t, with_efps, normed)
    else:
        kin, efp = _obs_cpu(t, with_efps, normed)
    return _out(kin, numpy_in), (None if efp is None else _out(efp, numpy_in))


def jet_features(jets) -> Dict[str, object]:
    """``jetnet.utils.jet_features``: ``{"pt", "eta", "phi", "mass"}`` of each jet's summed massless four-vectors."""
    kin, _ = _observables(jets, with_efps=False)
    return {k: kin[:, i] for i, k in enumerate(("pt", "eta", "phi", "mass"))}


_EFPSET_DEFAULT = (("n==", 4), ("d==", 4), ("p==", 1))
_EFPSET_D4 = (("d<=", 4),)


def efps(jets, normed: bool = True, efpset_args=None, efp_jobs=None):
    """``jetnet.utils.efps``.  ``efpset_args`` ``None`` or ``[("n==", 4), ("d==", 4), ("p==", 1)]`` (jetnet's default): ``[n, 5]``
    in the column order of the module docstring; ``[("d<=", 4)]`` (the set of ``fpd`` / ``kpd``): ``[n, 36]`` in the order of
    ``EFP_D4_GRAPHS``; any other set raises ``NotImplementedError``.  ``normed``: z_i = pT_i / sum pT (else pT_i);
    ``efp_jobs`` is accepted and unused (the EFPs run on the jets' device)."""
    spec = _EFPSET_DEFAULT if efpset_args is None else tuple(tuple(a) for a in efpset_args)
    if spec == _EFPSET_DEFAULT:
        return _observables(jets, with_efps=True, normed=normed)[1]
    if spec != _EFPSET_D4:
        raise NotImplementedError(f"mpgan_amd.evaluation has the EFP sets {list(_EFPSET_DEFAULT)} and {list(_EFPSET_D4)} "
                                  f"(got {list(spec)})")
    t, numpy_in = _as_tensor(jets)
    _check_jets(t)
    return _out(_efps_d4(t, normed), numpy_in)


# ------------------------------------------------------------------------------------- the 36 EFPs of degree <= 4
# The connected loopless multigraphs with at most 4 edges, in the column order of mpg_jet_efps_d4 (include/mpgan_amd.h)
_PRIME_GRAPHS = (
    (),                                      # 0  d = 0: one vertex
    ((0, 1),),                               # 1  edge
    ((0, 1), (0, 1)),                        # 2  double edge
    ((0, 1), (1, 2)),                        # 3  wedge
    ((0, 1), (0, 1), (0, 1)),                # 4  triple edge
    ((0, 1), (0, 1), (1, 2)),                # 5  a=b-c
    ((0, 1), (1, 2), (0, 2)),                # 6  triangle
    ((0, 1), (1, 2), (2, 3)),                # 7  path of 4 vertices
    ((0, 1), (0, 2), (0, 3)),                # 8  3-star
    ((0, 1), (0, 1), (0, 1), (0, 1)),        # 9  quadruple edge
    ((0, 1), (0, 1), (0, 1), (1, 2)),        # 10 triple edge + edge
    ((0, 1), (0, 1), (1, 2), (1, 2)),        # 11 two double edges sharing a vertex
    ((0, 1), (0, 1), (1, 2), (0, 2)),        # 12 triangle, one edge doubled
    ((0, 1), (0, 1), (1, 2), (2, 3)),        # 13 a=b-c-d            (column 0 of the five-EFP set)
    ((0, 1), (1, 2), (1, 2), (2, 3)),        # 14 a-b=c-d            (1)
    ((0, 1), (0, 1), (0, 2), (0, 3)),        # 15 3-star, one doubled (2)
    ((0, 1), (1, 2), (0, 2), (2, 3)),        # 16 triangle + pendant  (3)
    ((0, 1), (1, 2), (2, 3), (3, 0)),        # 17 4-cycle             (4)
    ((0, 1), (1, 2), (2, 3), (3, 4)),        # 18 path of 5 vertices
    ((0, 1), (0, 2), (0, 3), (0, 4)),        # 19 4-star
    ((0, 1), (0, 2), (0, 3), (3, 4)),        # 20 fork
)
NUM_EFP_D4_PRIMES = len(_PRIME_GRAPHS)       # MPG_JET_EFPS_D4_PRIMES of include/mpgan_amd.h
# the disconnected graphs of the set: multisets of the primes 1 .. 8 with at least two members and at most 4 edges in all
_COMPOSITE_FACTORS = ((1, 1), (1, 1, 1), (1, 2), (1, 3), (1, 1, 1, 1), (1, 1, 2), (1, 1, 3), (2, 2), (2, 3), (3, 3),
                      (1, 4), (1, 5), (1, 6), (1, 7), (1, 8))


def _disjoint_union(factors):
    edges, base = [], 0
    for f in factors:
        edges += [(a + base, b + base) for a, b in _PRIME_GRAPHS[f]]
        base += 1 + max(max(e) for e in _PRIME_GRAPHS[f])
    return tuple(edges)


# column k of ``efps(jets, efpset_args=[("d<=", 4)])`` is the EFP of the multigraph EFP_D4_GRAPHS[k] (a tuple of edges, pairs
# of vertex indices; () is the graph of one vertex and no edge) and the product of the prime columns EFP_D4_FACTORS[k]
EFP_D4_FACTORS = tuple((k,) for k in range(NUM_EFP_D4_PRIMES)) + _COMPOSITE_FACTORS
EFP_D4_GRAPHS = _PRIME_GRAPHS + tuple(_disjoint_union(f) for f in _COMPOSITE_FACTORS)
NUM_EFPS_D4 = len(EFP_D4_GRAPHS)


def _check_jets(t: torch.Tensor):
    if t.dim() != 3 or t.shape[2] < 3:
        raise ValueError(f"expected jets [n, N, >=3] = (eta_rel, phi_rel, pt_rel, ...), got {tuple(t.shape)}")
    if t.is_cuda and not 1 <= t.shape[1] <= MAX_PARTICLES:
        raise ValueError(f"mpg_jet_efps_d4 takes 1 <= N <= {MAX_PARTICLES} particles per jet (got {t.shape[1]})")


def _efp_primes_cuda(jets: torch.Tensor, normed: bool) -> torch.Tensor:
    """[n, 21] fp32 from mpg_jet_efps_d4."""
    n, N = jets.shape[0], jets.shape[1]
    if jets.dtype != torch.float32 or jets.stride(2) != 1:
        jets = jets.float().contiguous()
    out = torch.empty((n, NUM_EFP_D4_PRIMES), device=jets.device, dtype=torch.float32)
    if n == 0:
        return out
    with torch.cuda.device(jets.device):
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().mpg_jet_efps_d4(jets.data_ptr(), jets.stride(0), jets.stride(1), n, N,
                                              _FLAG_NORMED if normed else 0, out.data_ptr(), stream), "mpg_jet_efps_d4")
    return out


def _efp_primes_cpu(jets: torch.Tensor, normed: bool) -> torch.Tensor:
    """fp64 statement of mpg_jet_efps_d4 (the closed forms of include/mpgan_amd.h), chunked over jets."""
    x = jets[..., :3].double()
    n, N = x.shape[0], x.shape[1]
    out = torch.empty((n, NUM_EFP_D4_PRIMES), dtype=torch.float64)
    step = max(1, _CPU_CHUNK // max(1, N * N))
    for s in range(0, n, step):
        eta, phi, pt = x[s:s + step].unbind(-1)
        if normed:
            spt = pt.sum(1, keepdim=True)
            z = pt / torch.where(spt != 0, spt, 1.0)
        else:
            z = pt
        th = ((eta[:, :, None] - eta[:, None, :]) ** 2 + (phi[:, :, None] - phi[:, None, :]) ** 2).sqrt()
        th2 = th * th
        row = lambda A, y: torch.einsum("bij,bj->bi", A, y)
        w, T2, T3, T4 = row(th, z), row(th2, z), row(th2 * th, z), row(th2 * th2, z)
        zw = z * w
        v, q = row(th, zw), row(th2, zw)
        M = torch.einsum("bij,bj,bjk->bik", th, z, th)
        zMz = z[:, :, None] * M * z[:, None, :]
        cols = (z, zw, z * T2, zw * w, z * T3, z * T2 * w, None, zw * v, zw * w * w, z * T4, z * T3 * w, z * T2 * T2, None,
                z * T2 * v, zw * q, z * T2 * w * w, None, None, z * v * v, zw * w * w * w, zw * w * v)
        o = out[s:s + step]
        for k, c in enumerate(cols):
            if c is not None:
                o[:, k] = c.sum(1)
        o[:, 6] = (zMz * th).sum((1, 2))
        o[:, 12] = (zMz * th2).sum((1, 2))
        o[:, 16] = (zMz * th * w[:, None, :]).sum((1, 2))
        o[:, 17] = (zMz * M).sum((1, 2))
    return out


def _efps_d4(jets: torch.Tensor, normed: bool = True) -> torch.Tensor:
    """[n, 36] fp64 on the jets' device: the primes (fp32 from the kernel on a GPU, fp64 on the host), then their products."""
    primes = (_efp_primes_cuda(jets, normed) if jets.is_cuda else _efp_primes_cpu(jets, normed)).double()
    comps = [primes[:, list(f)].prod(1, keepdim=True) for f in _COMPOSITE_FACTORS]
    return torch.cat([primes] + comps, 1)


# ------------------------------------------------------------------------------------- W1
def wasserstein_1d(u, v) -> torch.Tensor:
    """``scipy.stats.wasserstein_distance(u, v)`` (the integral of |CDF_u - CDF_v|) in fp64 on the inputs' device:
    a 0-d tensor.  Samples may differ in size and hold ties."""
    u = torch.as_tensor(u).reshape(-1).double()
    v = torch.as_tensor(v, device=u.device).reshape(-1).double()
    us, vs = u.sort().values, v.sort().values
    allv = torch.cat([us, vs]).sort().values
    deltas = allv[1:] - allv[:-1]
    ucdf = torch.searchsorted(us, allv[:-1], right=True).double() / us.numel()
    vcdf = torch.searchsorted(vs, allv[:-1], right=True).double() / vs.numel()
    return ((ucdf - vcdf).abs() * deltas).sum()


def _draws(rng, n1: int, n2: int, k: int, device):
    rng = np.random if rng is None else rng
    i1 = rng.choice(n1, k)
    i2 = rng.choice(n2, k)
    return torch.from_numpy(np.asarray(i1)).to(device), torch.from_numpy(np.asarray(i2)).to(device)


def _batched_w1(x1: torch.Tensor, x2: torch.Tensor, num_eval_samples: int, num_batches: int, rng, per_column: bool):
    """W1 of ``num_batches`` random draws of ``x1`` against ``x2`` ([n, C] observables): [num_batches, C] float64."""
    out = []
    for _ in range(num_batches):
        i1, i2 = _draws(rng, x1.shape[0], x2.shape[0], num_eval_samples, x1.device)
        a, b = x1[i1], x2[i2]
        out.append(torch.stack([wasserstein_1d(a[:, c], b[:, c]) for c in range(a.shape[1])]) if per_column
                   else wasserstein_1d(a, b).reshape(1))
    return torch.stack(out).cpu().numpy()


def _mean_std(w1s: np.ndarray, average: bool, return_std: bool):
    means, stds = np.mean(w1s, axis=0), np.std(w1s, axis=0)
    if average:
        means, stds = np.mean(means), np.linalg.norm(stds)
    return (means, stds) if return_std else means


def _obs_tensor(x, like=None):
    t, _ = _as_tensor(x)
    return t.to(like.device) if like is not None else t


def w1m(jets1, jets2, num_eval_samples: int = 50000, num_batches: int = 5, return_std: bool = True, rng=None):
    """``jetnet.evaluation.w1m``: W1 of the jet mass, mean (and std) over ``num_batches`` draws of
    ``num_eval_samples`` jets from each set.  ``rng``: anything with numpy's ``choice`` (default: ``np.random``)."""
    m1 = _obs_tensor(jet_features(_obs_tensor(jets1))["mass"])
    m2 = _obs_tensor(jet_features(_obs_tensor(jets2, m1))["mass"])
    w1s = _batched_w1(m1[:, None], m2[:, None], num_eval_samples, num_batches, rng, per_column=False)[:, 0]
    return (float(np.mean(w1s)), float(np.std(w1s))) if return_std else float(np.mean(w1s))


def w1p(jets1, jets2, mask1=None, mask2=None, exclude_zeros: bool = True, num_particle_features: int = 0,
        num_eval_samples: int = 50000, num_batches: int = 5, average_over_features: bool = True, return_std: bool = True,
        rng=None):
    """``jetnet.evaluation.w1p``: W1 of each particle feature over the particles of ``num_eval_samples`` drawn jets per
    set and batch.  ``exclude_zeros`` drops particles whose feature vector has norm 0; ``mask1`` / ``mask2`` [n, N]
    select particles instead.  ``average_over_features=False``: per-feature means and stds (as the reference calls it)."""
    j1 = _obs_tensor(jets1)
    j2 = _obs_tensor(jets2, j1)
    F = num_particle_features if num_particle_features > 0 else j1.shape[2]
    j1, j2 = j1[:, :, :F], j2[:, :, :F]
    if mask1 is not None or mask2 is not None:
        mask1 = _obs_tensor(mask1, j1).bool().reshape(j1.shape[:2]) if mask1 is not None else torch.ones(j1.shape[:2], dtype=torch.bool, device=j1.device)
        mask2 = _obs_tensor(mask2, j1).bool().reshape(j2.shape[:2]) if mask2 is not None else torch.ones(j2.shape[:2], dtype=torch.bool, device=j1.device)
    elif exclude_zeros:
        mask1 = j1.double().norm(dim=2) != 0
        mask2 = j2.double().norm(dim=2) != 0
    w1s = []
    for _ in range(num_batches):
        i1, i2 = _draws(rng, j1.shape[0], j2.shape[0], num_eval_samples, j1.device)
        p1 = j1[i1][mask1[i1]] if mask1 is not None else j1[i1].reshape(-1, F)
        p2 = j2[i2][mask2[i2]] if mask2 is not None else j2[i2].reshape(-1, F)
        if p1.shape[0] == 0 or p2.shape[0] == 0:
            w1s.append(np.full(F, np.inf))
        else:
            w1s.append(torch.stack([wasserstein_1d(p1[:, f], p2[:, f]) for f in range(F)]).cpu().numpy())
    return _mean_std(np.stack(w1s), average_over_features, return_std)


def w1efp(jets1, jets2, use_particle_masses: bool = False, num_eval_samples: int = 50000, num_batches: int = 5,
          average_over_efps: bool = True, return_std: bool = True, efp_jobs=None, normed: bool = True, rng=None):
    """``jetnet.evaluation.w1efp`` with its default EFP set: W1 of each of the five EFPs (``efps``).  Massless particles
    only (``use_particle_masses=True`` raises); ``efp_jobs`` is accepted and unused (the EFPs run on the jets' device)."""
    if use_particle_masses:
        raise NotImplementedError("mpgan_amd.evaluation computes EFPs of massless particles only")
    e1 = _obs_tensor(efps(_obs_tensor(jets1), normed=normed))
    e2 = _obs_tensor(efps(_obs_tensor(jets2, e1), normed=normed))
    w1s = _batched_w1(e1, e2, num_eval_samples, num_batches, rng, per_column=True)
    return _mean_std(w1s, average_over_efps, return_std)


# ------------------------------------------------------------------------------------- EMD, coverage and MMD
_HOST_THREADS = 16


def _emd_input(t: torch.Tensor, width: int) -> torch.Tensor:
    """fp32, contiguous [n, N, width] (width 3, or the callers' common width: a fourth mask column is stepped over)."""
    if t.dtype != torch.float32 or not t.is_contiguous() or t.shape[2] != width:
        t = t[..., :3].float().contiguous()
    return t


def _emds(a: torch.Tensor, b: torch.Tensor, R: float) -> torch.Tensor:
    """[n1, n2] distances on a's device (fp32 through mpg_jet_emd on a GPU, fp64 through mpg_jet_emd_host otherwise);
    raises when a pair did not finish inside the solver's cap."""
    for t in (a, b):
        if t.dim() != 3 or t.shape[2] < 3:
            raise ValueError(f"expected jets [n, N, >=3] = (eta_rel, phi_rel, pt_rel, ...), got {tuple(t.shape)}")
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"both sets must hold the same number of particle slots per jet (got {a.shape[1]} and {b.shape[1]})")
    width = a.shape[2] if a.shape[2] == b.shape[2] else 3
    a, b = _emd_input(a, width), _emd_input(b.to(a.device), width)
    n1, n2, N, ld = a.shape[0], b.shape[0], a.shape[1], a.shape[2]
    if not 1 <= N <= MAX_PARTICLES:
        raise ValueError(f"mpg_jet_emd takes 1 <= N <= {MAX_PARTICLES} particles per jet (got {N})")
    if not R > 0:
        raise ValueError(f"R must be positive (got {R})")
    out = torch.empty((n1, n2), device=a.device, dtype=torch.float32 if a.is_cuda else torch.float64)
    if n1 == 0 or n2 == 0:
        return out
    status = torch.empty((n1, n2), device=a.device, dtype=torch.int32)
    if a.is_cuda:
        with torch.cuda.device(a.device):
            stream = torch.cuda.current_stream().cuda_stream
            _lib.check(_lib.lib().mpg_jet_emd(a.data_ptr(), N * ld, b.data_ptr(), N * ld, ld, n1, n2, N, float(R),
                                              out.data_ptr(), status.data_ptr(), stream), "mpg_jet_emd")
    else:
        _lib.check(_lib.lib().mpg_jet_emd_host(a.data_ptr(), N * ld, b.data_ptr(), N * ld, ld, n1, n2, N, float(R),
                                               out.data_ptr(), status.data_ptr(), _HOST_THREADS), "mpg_jet_emd_host")
    bad = int((status != 0).sum())
    if bad:
        raise RuntimeError(f"mpg_jet_emd: {bad} of {n1 * n2} pairs did not reach the optimum (status "
                           f"{sorted(set(status[status != 0].flatten().tolist()))}: 1 = augmentation cap, 2 = no path, "
                           f"non-finite input)")
    return out


def emds(jets1, jets2, R: float = 1.0):
    """``[n1, n2]`` energy mover's distances ``EMD(jets1[i], jets2[j])`` (module docstring): fp32 on the GPU for CUDA tensors,
    fp64 on the host for CPU tensors and numpy arrays (numpy in, numpy out)."""
    a, numpy_in = _as_tensor(jets1)
    b, _ = _as_tensor(jets2)
    return _out(_emds(a, b, R), numpy_in)


def cov_mmd(real_jets, gen_jets, num_eval_samples: int = 100, num_batches: int = 10, rng=None):
    """``jetnet.evaluation.cov_mmd``: ``(coverage, mmd)`` as floats, means over ``num_batches`` batches of
    ``num_eval_samples`` jets drawn from each set (module docstring).  ``rng``: anything with numpy's ``choice``."""
    real = _obs_tensor(real_jets)
    gen = _obs_tensor(gen_jets, real)
    covs, mmds = [], []
    for _ in range(num_batches):
        i_real, i_gen = _draws(rng, real.shape[0], gen.shape[0], num_eval_samples, real.device)
        D = _emds(gen[i_gen], real[i_real], 1.0)              # [gen, real]
        mmds.append(D.min(dim=0).values.double().mean())
        covs.append(torch.unique(_first_argmin(D)).numel() / num_eval_samples)
    return float(np.mean(covs)), float(torch.stack(mmds).mean())


def _first_argmin(D: torch.Tensor) -> torch.Tensor:
    """numpy's argmin along the rows of D: the first index of each row's minimum."""
    n = D.shape[1]
    idx = torch.arange(n, device=D.device).expand_as(D)
    return torch.where(D == D.min(dim=1, keepdim=True).values, idx, n).min(dim=1).values


# ------------------------------------------------------------------------------------- FPD and KPD
def _np64(x) -> np.ndarray:
    return x.detach().cpu().double().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)


def _psd_sqrt(s: np.ndarray) -> np.ndarray:
    lam, V = np.linalg.eigh(0.5 * (s + s.T))
    return (V * np.sqrt(np.clip(lam, 0, None))) @ V.T


def frechet_distance(mu1, sigma1, mu2, sigma2) -> float:
    """|mu1 - mu2|^2 + Tr(S1) + Tr(S2) - 2 Tr sqrt(S1 S2) between two Gaussians, in fp64 on the host.  The eigenvalues of S1 S2
    are those of the symmetric positive semi-definite S1^{1/2} S2 S1^{1/2} = A A^T with A = S1^{1/2} S2^{1/2} (symmetric roots
    from ``eigh``, eigenvalues clamped at 0), so Tr sqrt(S1 S2) is the sum of A's singular values: no complex parts, no scipy.
    They are taken from an SVD of A rather than as square roots of computed eigenvalues of A A^T: the covariances of the 36
    EFPs have eigenvalues down to 1e-10 of the largest, an eigen-solver leaves an absolute error of 1e-16 |A A^T| in each
    eigenvalue, and the square root of an eigenvalue below that is noise of 1e-8 |A| -- the SVD's error is 1e-16 |A|.
    A column whose variance is exactly 0 in either set (the degree-0 EFP of normed jets) has a zero row and column in that
    covariance and hence in A A^T: it is left out of the roots, which changes nothing but the rounding."""
    mu1, mu2 = _np64(mu1).reshape(-1), _np64(mu2).reshape(-1)
    s1, s2 = np.atleast_2d(_np64(sigma1)), np.atleast_2d(_np64(sigma2))
    d = mu1 - mu2
    keep = (np.diag(s1) > 0) & (np.diag(s2) > 0)
    tr_sqrt = 0.0
    if keep.any():
        A = _psd_sqrt(s1[np.ix_(keep, keep)]) @ _psd_sqrt(s2[np.ix_(keep, keep)])
        tr_sqrt = float(np.linalg.svd(A, compute_uv=False).sum())
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2 * tr_sqrt)


def _mean_cov(x: torch.Tensor):
    """Mean and covariance (``np.cov(x, rowvar=False)``: divided by rows - 1) of fp64 rows, on their device."""
    mu = x.mean(0)
    c = x - mu
    return mu, c.T @ c / (x.shape[0] - 1)


def _feature_pair(real_features, gen_features, normalise: bool):
    """Both sets as fp64 tensors on the real features' device; ``normalise`` divides both by max |real| of each column (jetnet's
    ``_normalise_features``; a column that is 0 throughout is left as it is instead of becoming NaN)."""
    X = _obs_tensor(real_features).double()
    Y = _obs_tensor(gen_features, X).double()
    if X.dim() != 2 or Y.dim() != 2 or X.shape[1] != Y.shape[1]:
        raise ValueError(f"expected features [n, F] and [m, F], got {tuple(X.shape)} and {tuple(Y.shape)}")
    if normalise:
        top = X.abs().max(0).values
        top = torch.where(top > 0, top, torch.ones_like(top))
        X, Y = X / top, Y / top
    return X, Y


def _bounded_line_fit(x: np.ndarray, y: np.ndarray):
    """Least squares of ``y = intercept + slope * x`` with both parameters >= 0: (intercept, slope, standard error of the
    intercept).  The objective is a convex quadratic in two variables, so the minimum over the quadrant is the unconstrained
    one when that lies inside, else the better of the two one-parameter fits on the boundary.  The error is what
    ``scipy.optimize.curve_fit`` reports: the square root of RSS / (points - 2) (J^T J)^{-1}[0, 0] with J = [1, x]."""
    A = np.stack([np.ones_like(x), x], 1)
    (a, b), *_ = np.linalg.lstsq(A, y, rcond=None)
    if a < 0 or b < 0:
        cands = [(max(float(y.mean()), 0.0), 0.0), (0.0, max(float(x @ y / (x @ x)), 0.0))]
        a, b = min(cands, key=lambda ab: float(((y - ab[0] - ab[1] * x) ** 2).sum()))
    rss = float(((y - a - b * x) ** 2).sum())
    dof = len(x) - 2
    err = float(np.sqrt(rss / dof * np.linalg.inv(A.T @ A)[0, 0])) if dof > 0 else float("inf")
    return float(a), float(b), err


def fpd(real_features, gen_features, min_samples: int = 20000, max_samples: int = 50000, num_batches: int = 20,
        num_points: int = 10, normalise: bool = True, seed: int = 42, rng=None):
    """``jetnet.evaluation.fpd`` (Frechet physics distance, Kansal et al. 2022) of two feature sets ``[n, F]``, e.g.
    ``efps(jets, efpset_args=[("d<=", 4)])``: ``(value, error)``, the Frechet distance between Gaussians fitted to the two sets
    extrapolated to infinite sample size.  Restated from memory of jetnet: batch sizes
    ``(1 / linspace(1 / min_samples, 1 / max_samples, num_points)).astype(int32)``; for each size the mean over ``num_batches``
    of ``frechet_distance`` between ``real[rng.choice(len(real), size)]`` and ``gen[rng.choice(len(gen), size)]`` (real drawn
    first, with replacement); a least-squares line ``intercept + slope / size`` with both parameters >= 0; the intercept and
    its standard error are returned.  jetnet reseeds numpy's GLOBAL stream with ``seed``; here the draws come from a private
    ``np.random.RandomState(seed)`` -- the same numbers, without disturbing the draws of other metrics -- or from ``rng`` when
    given.  Means and covariances are computed in fp64 on the features' device, the F x F eigenproblems on the host."""
    X, Y = _feature_pair(real_features, gen_features, normalise)
    rng = np.random.RandomState(seed) if rng is None else rng
    sizes = (1 / np.linspace(1.0 / min_samples, 1.0 / max_samples, num_points)).astype("int32")
    vals = []
    for size in sizes:
        points = []
        for _ in range(num_batches):
            i1, i2 = _draws(rng, X.shape[0], Y.shape[0], int(size), X.device)
            points.append(frechet_distance(*_mean_cov(X[i1]), *_mean_cov(Y[i2])))
        vals.append(np.mean(points))
    intercept, _, err = _bounded_line_fit(1.0 / sizes.astype(np.float64), np.asarray(vals, dtype=np.float64))
    return intercept, err


_KPD_ROWS = 1024             # rows per chunk of a kernel matrix (1024 x 5000 fp64: 41 MB)


def _poly_kernel_sum(A: torch.Tensor, B: torch.Tensor, degree: int) -> torch.Tensor:
    """sum_ij (A_i . B_j / F + 1)^degree in fp64, the kernel matrix formed ``_KPD_ROWS`` rows at a time."""
    F = A.shape[1]
    return torch.stack([((A[s:s + _KPD_ROWS] @ B.T / F + 1.0) ** degree).sum() for s in range(0, A.shape[0], _KPD_ROWS)]).sum()


def _mmd_poly_unbiased(X: torch.Tensor, Y: torch.Tensor, degree: int) -> float:
    m, n, F = X.shape[0], Y.shape[0], X.shape[1]
    diag = lambda A: (((A * A).sum(1) / F + 1.0) ** degree).sum()
    xx = (_poly_kernel_sum(X, X, degree) - diag(X)) / (m * (m - 1))
    yy = (_poly_kernel_sum(Y, Y, degree) - diag(Y)) / (n * (n - 1))
    xy = _poly_kernel_sum(X, Y, degree) / (m * n)
    return float(xx + yy - 2 * xy)


def kpd(real_features, gen_features, num_batches: int = 10, batch_size: int = 5000, degree: int = 4, normalise: bool = True,
        seed: int = 42, rng=None):
    """``jetnet.evaluation.kpd`` (kernel physics distance): ``(median, error)`` over ``num_batches`` batches of the unbiased
    quadratic MMD ``(sum K_XX - tr K_XX) / (m (m - 1)) + (sum K_YY - tr K_YY) / (m (m - 1)) - 2 mean K_XY`` between
    ``batch_size`` rows drawn from each set (real first, with replacement), with the polynomial kernel
    ``K(x, y) = (x . y / F + 1)^degree``, F the number of columns; the error is half the 16.275 - 83.725 percentile range
    (numpy's linear interpolation).  Restated from memory of jetnet, like ``fpd``: the paper describes the kernel as cubic, the
    code as remembered has ``degree = 4``, which is therefore the default here; pass ``degree=3`` for the paper's.  Draws come
    from a private ``np.random.RandomState(seed)`` or from ``rng`` (see ``fpd``).  fp64 on the features' device: the three sums
    cancel to 1e-3 .. 1e-6 of their size."""
    X, Y = _feature_pair(real_features, gen_features, normalise)
    rng = np.random.RandomState(seed) if rng is None else rng
    vals = []
    for _ in range(num_batches):
        i1, i2 = _draws(rng, X.shape[0], Y.shape[0], batch_size, X.device)
        vals.append(_mmd_poly_unbiased(X[i1], Y[i2], degree))
    lo, hi = np.percentile(vals, [16.275, 83.725])
    return float(np.median(vals)), float(hi - lo) / 2


# ------------------------------------------------------------------------------------- the reference's evaluate
def evaluate(losses: dict, real_jets, gen_jets, jet_type: str, num_particles: int = 30, num_w1_eval_samples: int = 10000,
             num_cov_mmd_eval_samples: int = 100, num_fpnd_eval_samples: int = 50000, fpnd_batch_size: int = 16,
             efp_jobs=None, real_efps=None, gen_efps=None, rng=None, *, fpd_args: Optional[dict] = None,
             kpd_args: Optional[dict] = None):
    """train.py:543-606: append ``w1p`` (means(3) then stds(3)), ``w1m`` ([mean, std]) and ``w1efp`` (means(5) then
    stds(5)) to the lists of ``losses`` that hold those keys, with ``len(real_jets) // num_w1_eval_samples`` batches.
    ``"fpd"`` and ``"kpd"`` get ``np.array([value, error])`` of ``fpd`` / ``kpd`` only when ``real_efps`` and ``gen_efps`` (the
    ``[n, 36]`` of ``efps(jets, efpset_args=[("d<=", 4)])``) are given -- the reference's evaluate carries that line commented
    out and train.py:604-606 appends after it; without them both keys are left alone.  They come last and draw from their own
    ``RandomState(seed)`` (``fpd_args`` / ``kpd_args`` are passed on as keyword arguments), so every other key's draws are
    what they are without them.  ``"fpnd"`` raises ``NotImplementedError``.
    The draws come from ``rng`` (default ``np.random``) in the reference's order: w1p, w1m, w1efp.  ``"coverage"`` and
    ``"mmd"`` (``cov_mmd`` with ``num_cov_mmd_eval_samples`` samples, 10 batches) are appended after those three, so the draws
    of a caller without these keys are what they were."""
    if "fpnd" in losses:
        raise NotImplementedError("fpnd needs jetnet's pretrained ParticleNet, which mpgan_amd does not provide")
    num_batches = len(real_jets) // num_w1_eval_samples
    if "w1p" in losses:
        m, s = w1p(real_jets, gen_jets, exclude_zeros=True, num_eval_samples=num_w1_eval_samples, num_batches=num_batches,
                   average_over_features=False, return_std=True, rng=rng)
        losses["w1p"].append(np.concatenate((m, s)))
    if "w1m" in losses:
        m, s = w1m(real_jets, gen_jets, num_eval_samples=num_w1_eval_samples, num_batches=num_batches, return_std=True,
                   rng=rng)
        losses["w1m"].append(np.array([m, s]))
    if "w1efp" in losses:
        m, s = w1efp(real_jets, gen_jets, use_particle_masses=False, num_eval_samples=num_w1_eval_samples,
                     num_batches=num_batches, average_over_efps=False, return_std=True, efp_jobs=efp_jobs, rng=rng)
        losses["w1efp"].append(np.concatenate((m, s)))
    if "coverage" in losses or "mmd" in losses:
        cov, mmd = cov_mmd(real_jets, gen_jets, num_eval_samples=num_cov_mmd_eval_samples, rng=rng)
        if "coverage" in losses:
            losses["coverage"].append(cov)
        if "mmd" in losses:
            losses["mmd"].append(mmd)
    if real_efps is not None and gen_efps is not None:
        if "fpd" in losses:
            losses["fpd"].append(np.array(fpd(real_efps, gen_efps, **(fpd_args or {}))))
        if "kpd" in losses:
            losses["kpd"].append(np.array(kpd(real_efps, gen_efps, **(kpd_args or {}))))
    return losses


def evaluate_generator(G: torch.nn.Module, real_jets, jet_type: str, num_samples: int = 50000,
                       keys: Sequence[str] = ("w1p", "w1m"), losses: Optional[dict] = None, num_particles: int = 30,
                       num_w1_eval_samples: int = 10000, labels: Optional[torch.Tensor] = None, model: str = "mpgan",
                       model_args: Optional[dict] = None, batch_size: int = 4096, rng=None,
                       num_cov_mmd_eval_samples: int = 100, real_efps=None, fpd_args: Optional[dict] = None,
                       kpd_args: Optional[dict] = None, sampler=None) -> dict:
    """Generate ``num_samples`` jets with ``gen.generate_jets`` and ``evaluate`` them against ``real_jets`` ([n, N, >=3]
    un-normalised), all on G's device.  ``sampler``: a ``gen.JetSampler`` built on ``G`` -- the generated jets are then the next
    ``num_samples`` rows of its stream (labels drawn from its table; ``labels``, ``model``, ``model_args`` and ``batch_size``
    are not used); a sampler with a process group generates them over its ranks (``sample_all``: every rank calls this function
    and gets the same result).  ``labels`` (num_particles / N per generated jet) default to the multiplicities of
    the real jets, taken in order and repeated as needed -- the reference conditions on the test set's ``jet_data``
    (train.py:712-723).  With ``"fpd"`` or ``"kpd"`` among the keys the 36 EFPs of degree <= 4 of the generated jets are computed
    on the device, and those of the real jets unless ``real_efps`` carries them (train.py:744-755 keeps them in a file per jet
    type).  Returns ``losses`` (a new ``{key: []}`` for ``keys`` when not given) with one entry appended."""
    from .gen import generate_jets
    device = next(G.parameters()).device
    real, _ = _as_tensor(real_jets)
    real = real.to(device)
    N = real.shape[1]
    if sampler is not None:
        if sampler.G is not G or sampler.N != N or sampler.jet_type != jet_type:
            raise ValueError(f"evaluate_generator: the sampler generates {sampler.jet_type!r} jets of {sampler.N} particles from its own "
                             f"generator; asked for {jet_type!r} jets of {N} particles from G")
        # (a sampler of several ranks: every rank generates its chunks and all of them evaluate the gathered rows -- a collective)
        gen_jets = sampler.sample_all(num_samples) if getattr(sampler, "pg", None) is not None else sampler.sample(num_samples)
        gen_jets = gen_jets[0] if isinstance(gen_jets, tuple) else gen_jets
    else:
        if labels is None:
            idx = torch.arange(num_samples, device=device) % real.shape[0]
            labels = ((real[idx, :, 2] != 0).sum(1).float() * np.float32(1.0 / N)).reshape(-1, 1)
        gen_jets = generate_jets(G, num_samples, num_particles=N, labels=labels, jet_type=jet_type, model=model,
                                 model_args=model_args, batch_size=batch_size)
    if losses is None:
        losses = {k: [] for k in keys}
    gen_efps = None
    if "fpd" in losses or "kpd" in losses:
        gen_efps = _efps_d4(gen_jets)
        real_efps = _efps_d4(real) if real_efps is None else _obs_tensor(real_efps, gen_efps)
    return evaluate(losses, real[..., :3], gen_jets, jet_type, num_particles=num_particles,
                    num_w1_eval_samples=num_w1_eval_samples, num_cov_mmd_eval_samples=num_cov_mmd_eval_samples, rng=rng,
                    real_efps=real_efps if gen_efps is not None else None, gen_efps=gen_efps, fpd_args=fpd_args,
                    kpd_args=kpd_args)
