"""Jet data in the layout the hot path consumes, without the JetNet package.

The reference feeds ``train_D`` batches ``data [B, N, 4] = (eta_rel, phi_rel, pT_rel, mask)`` normalised by
``FeaturewiseLinearBounded(feature_norms=1, feature_shifts=[0, 0, -0.5, -0.5], feature_maxes=fpnd maxes + [1])``
and ``labels [B, 1] = num_particles / N`` (``train.py:36-67``); ``gen.py:127-139`` undoes that normalisation on
generated jets.  This module holds

* ``synthetic_jets``   -- the synthetic stand-in for JetNet used by bench.py and the tests,
* ``normalise_jets`` / ``unnormalise_jets`` -- the two directions of the reference's feature normalisation,
* ``JetArrayDataset``  -- a ``torch.utils.data.Dataset`` over raw ``[n, N, 4]`` particle arrays, yielding
  ``(data, labels)`` exactly as ``train.py:843-846`` unpacks them,
* ``read_jetnet_file`` / ``JetArrayDataset.from_jetnet_file`` -- the reader of JetNet's on-disk layout
  (``<data_dir>/<jet_type>[150].hdf5`` with the datasets ``particle_features [n, N, 4]`` = (etarel, phirel, ptrel, mask)
  and ``jet_features [n, 4]`` = (pt, eta, mass, num_particles), jetnet >= 0.2.1 as ``requirements.txt:2`` pins it; the
  same two arrays in an ``.npz`` are read alike),
* ``DeviceJetLoader`` -- the whole data set resident on the training device, shuffled by a keyed permutation and gathered into
  ``TrainStep``'s buffers by one launch inside the captured iteration (``TrainStep(loader=...)``).
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

# maxima of (eta_rel, phi_rel, pT_rel, mask) per jet type: gen.py:10-14 (= JetNet.fpnd_norm.feature_maxes + [1])
FEATURE_MAXES = {
    "g": [1.4532885551452637, 0.520724892616272, 0.8537549376487732, 1.0],
    "q": [1.6211985349655151, 0.4568111002445221, 0.8896132111549377, 1.0],
    "t": [1.4242753982543945, 0.4949831962585449, 0.8774275183677673, 1.0],
}
FEATURE_NORMS = [1.0, 1.0, 1.0, 1.0]       # gen.py:16
FEATURE_SHIFTS = [0.0, 0.0, -0.5, -0.5]    # gen.py:17, train.py:43


def synthetic_jets(B: int, N: int, seed: int = 4, dist: str = "gluon", dtype=torch.float32):
    """``(data [B,N,4], labels [B,1])`` of synthetic JetNet-like jets, already normalised.

    Multiplicity n per jet: ``gluon`` = clip(round(Normal(0.8 N, 0.15 N)), 1, N), ``uniform`` = UniformInt[1, N]; ``top`` =
    clip(round(Normal(0.95 N, 0.08 N)), 1, N) and ``quark`` = clip(round(Normal(0.7 N, 0.18 N)), 1, N) -- stand-ins for the
    other two jet types of the reference's ``--jets`` (top jets have more constituents than gluon jets, so nearly all fill the
    N leading-pT slots; light-quark jets fewer); the dataset itself is not available here, the laws only shape the work.
    The first n particles are real: eta_rel, phi_rel ~ clip(Normal(0, 0.15), -1, 1), pT_rel ~ Uniform(-0.5, 0.5),
    mask = +0.5; padding particles are (0, 0, -0.5, -0.5).  ``labels = float32(n) * float32(1/N)`` -- the product
    with the reciprocal makes ``int(labels * N)`` return n for every n <= 150, n / N does not."""
    rs = np.random.RandomState(seed)
    if dist == "uniform":
        n = rs.randint(1, N + 1, size=B)
    elif dist == "gluon":
        n = np.clip(np.rint(rs.normal(0.8 * N, 0.15 * N, size=B)), 1, N).astype(np.int64)
    elif dist == "top":
        n = np.clip(np.rint(rs.normal(0.95 * N, 0.08 * N, size=B)), 1, N).astype(np.int64)
    elif dist == "quark":
        n = np.clip(np.rint(rs.normal(0.7 * N, 0.18 * N, size=B)), 1, N).astype(np.int64)
    else:
        raise ValueError(f"unknown multiplicity law {dist!r}")
    eta = np.clip(rs.normal(0, 0.15, size=(B, N)), -1, 1)
    phi = np.clip(rs.normal(0, 0.15, size=(B, N)), -1, 1)
    pt = rs.uniform(-0.5, 0.5, size=(B, N))
    real = np.arange(N)[None, :] < n[:, None]
    pad = (0.0, 0.0, -0.5, -0.5)
    data = np.stack([np.where(real, f, v) for f, v in zip((eta, phi, pt, np.full((B, N), 0.5)), pad)], axis=2)
    labels = (n.astype(np.float32) * np.float32(1.0 / N)).reshape(B, 1)
    return torch.from_numpy(data).to(dtype), torch.from_numpy(labels).to(dtype)


def normalise_jets(raw: torch.Tensor, jet_type: str = "g") -> torch.Tensor:
    """Raw ``(eta_rel, phi_rel, pT_rel[, mask])`` -> the network's input range: x / max * norm + shift per feature
    (``FeaturewiseLinearBounded`` as configured at ``train.py:41-45``)."""
    F = raw.shape[-1]
    mx = raw.new_tensor(FEATURE_MAXES[jet_type][:F])
    return raw / mx * raw.new_tensor(FEATURE_NORMS[:F]) + raw.new_tensor(FEATURE_SHIFTS[:F])


def unnormalise_jets(gen_jets: torch.Tensor, jet_type: str = "g", mask: bool = True) -> torch.Tensor:
    """The epilogue of the reference's ``gen.py:127-141`` on generator output ``[n, N, 3 (+ mask)]``: undo shift /
    norm / max on the three particle features, zero the particles whose mask feature is below 0.5 (the generator
    emits mask - 0.5, so that is "mask bit clear" exactly as gen.py tests it), clamp pT_rel at 0, drop the mask
    column.  Returns a new ``[n, N, 3]`` tensor."""
    out = gen_jets[..., :3].clone()
    for i in range(3):
        if FEATURE_SHIFTS[i]:
            out[..., i] -= FEATURE_SHIFTS[i]
        out[..., i] /= FEATURE_NORMS[i]
        out[..., i] *= FEATURE_MAXES[jet_type][i]
    if mask:
        out[~(gen_jets[..., -1] >= 0.5)] = 0
    out[..., 2].clamp_(min=0)
    return out


JETNET_PARTICLE_FEATURES = ("etarel", "phirel", "ptrel", "mask")      # JetNet.all_particle_features
JETNET_JET_FEATURES = ("pt", "eta", "mass", "num_particles")           # JetNet.all_jet_features


def read_jetnet_file(path: str):
    """``(particle_features [n, N, 4] float32, jet_features [n, 4] float32 or None)`` of a JetNet data file.

    ``.hdf5`` / ``.h5``: the datasets ``particle_features`` and ``jet_features`` of jetnet's own files (needs ``h5py``, which
    is what jetnet itself reads them with; a clear error says so when it is missing).  ``.npz``: the same two keys
    (``jet_features`` optional).  ``.npy``: the particle array alone."""
    import os
    ext = os.path.splitext(path)[1].lower()
    if ext in (".hdf5", ".h5"):
        try:
            import h5py
        except ImportError as e:  # pragma: no cover - depends on the environment
            raise ImportError(f"reading {path} needs h5py (JetNet's files are HDF5); export the two datasets "
                              "'particle_features' and 'jet_features' to an .npz to read them without it") from e
        with h5py.File(path, "r") as f:
            pf = np.asarray(f["particle_features"], dtype=np.float32)
            jf = np.asarray(f["jet_features"], dtype=np.float32) if "jet_features" in f else None
    elif ext == ".npz":
        with np.load(path) as f:
            if "particle_features" not in f.files:
                raise KeyError(f"{path}: no 'particle_features' array (found {f.files})")
            pf = np.asarray(f["particle_features"], dtype=np.float32)
            jf = np.asarray(f["jet_features"], dtype=np.float32) if "jet_features" in f.files else None
    elif ext == ".npy":
        pf, jf = np.asarray(np.load(path), dtype=np.float32), None
    else:
        raise ValueError(f"{path}: expected .hdf5 / .h5 / .npz / .npy")
    if pf.ndim != 3 or pf.shape[-1] != len(JETNET_PARTICLE_FEATURES):
        raise ValueError(f"{path}: particle_features has shape {pf.shape}, expected [n, N, 4] = {JETNET_PARTICLE_FEATURES}")
    if jf is not None and (jf.ndim != 2 or jf.shape[0] != pf.shape[0] or jf.shape[1] != len(JETNET_JET_FEATURES)):
        raise ValueError(f"{path}: jet_features has shape {jf.shape}, expected [{pf.shape[0]}, 4] = {JETNET_JET_FEATURES}")
    return pf, jf


class JetArrayDataset(torch.utils.data.Dataset):
    """Raw JetNet-style particle arrays ``[n, N, 4] = (eta_rel, phi_rel, pT_rel, mask in {0, 1})`` served the way
    ``train.py``'s ``DataLoader`` serves JetNet: item = ``(normalised particles [N, 4], label [1])`` with
    label = num_particles / N (``jet_normalisation``: ``FeaturewiseLinear(feature_scales=1 / num_hits)``)."""

    def __init__(self, particles, jet_type: str = "g", num_particles: Optional[int] = None,
                 split: str = "train", split_fraction: Sequence[float] = (0.7, 0.3, 0.0), multiplicities=None):
        """``particles``: an array ``[n, N, 4]`` or a file ``read_jetnet_file`` understands.  ``multiplicities`` ``[n]``: the
        ``num_particles`` jet feature when it comes from a file; by default (and always when the particle axis is cut to
        ``num_particles``) it is counted from the mask column, which is what JetNet's own column holds."""
        if isinstance(particles, str):
            particles, jf = read_jetnet_file(particles)
            if multiplicities is None and jf is not None:
                multiplicities = jf[:, JETNET_JET_FEATURES.index("num_particles")]
        p = torch.as_tensor(np.asarray(particles), dtype=torch.float32)
        if p.dim() != 3 or p.shape[-1] != 4:
            raise ValueError(f"expected particle features [n, N, 4], got {tuple(p.shape)}")
        if num_particles is not None and num_particles < p.shape[1]:
            p = p[:, :num_particles]
            multiplicities = None        # the first num_particles (pT-ordered) particles: count again
        n = p.shape[0]
        cuts = np.cumsum([0] + [int(round(f * n)) for f in split_fraction])
        k = {"train": 0, "valid": 1, "test": 2, "all": None}[split]
        lo, hi = (0, n) if k is None else (int(cuts[k]), int(min(cuts[k + 1], n)))
        p = p[lo:hi]
        self.num_particles = p.shape[1]
        if multiplicities is None:
            mult = p[..., 3].sum(1, keepdim=True)
        else:
            mult = torch.as_tensor(np.asarray(multiplicities), dtype=torch.float32).reshape(-1, 1)[lo:hi]
        # jet_normalisation = FeaturewiseLinear(feature_scales = 1 / num_hits) (train.py:46): the PRODUCT with the reciprocal
        self.jet_features = (mult * np.float32(1.0 / self.num_particles)).float()
        self.particle_data = normalise_jets(p, jet_type)

    @classmethod
    def from_jetnet_file(cls, data_dir: str, jet_type: str = "g", num_particles: int = 30, split: str = "train",
                         split_fraction: Sequence[float] = (0.7, 0.3, 0.0)):
        """The dataset ``JetNet(jet_type, data_dir, num_particles, particle_features = all, jet_features = "num_particles",
        particle_normalisation, jet_normalisation, split_fraction, split)`` of ``train.py:47-64`` from jetnet's file in
        ``data_dir``: ``<jet_type>.hdf5`` (30 particles) or ``<jet_type>150.hdf5`` (more), else the same stem as ``.npz``."""
        import os
        stem = jet_type + ("150" if num_particles > 30 else "")
        for ext in (".hdf5", ".h5", ".npz"):
            path = os.path.join(data_dir, stem + ext)
            if os.path.isfile(path):
                return cls(path, jet_type=jet_type, num_particles=num_particles, split=split, split_fraction=split_fraction)
        raise FileNotFoundError(f"no {stem}.hdf5 / .h5 / .npz in {data_dir}")

    def __len__(self):
        return self.particle_data.shape[0]

    def __getitem__(self, i):
        return self.particle_data[i], self.jet_features[i]


LOADER_KEY_TERM = 0xA0761D6478BD642F   # what tells the shuffle's key from the noise / dropout seed derived from the same torch seed


class DeviceJetLoader:
    """A data set held on the training device and fed to ``train.TrainStep`` without the host: ``particle_data [n, N, 4]`` and
    ``jet_features [n, 1]`` (a ``JetArrayDataset``, or the two arrays as a pair) stay on ``device``; the jets are visited in the
    order of a keyed shuffle (``perm(key, epoch, i, n)`` of include/mpgan_amd.h: a function of the key and the position, no
    permutation buffer) and one launch (``mpg_batch_feed``) gathers a batch into the step's buffers and moves the cursor on.

    The stream of positions is continuous: position g takes row ``perm(key, g // n, g % n, n)``.  No batch is dropped or short
    (``DataLoader(shuffle=True)`` ends an epoch on a short batch; a captured iteration has one batch size): a batch may
    straddle two epochs, and every n consecutive positions from a multiple of n visit every jet once.

    ``seed`` (default ``torch.initial_seed()``) gives the key -- NOT the rank: all ranks share one shuffle and take disjoint
    slices of it, rank r of W starting at r * batch_size and striding by W * batch_size, so that together they consume the stream
    contiguously (no ``DistributedSampler``).  ``state_dict()`` is the whole state of the data order: saved beside the
    optimizers' state it makes a resumed run see the jets an uninterrupted one would.

    CPU tensors (host-logic tests with toy modules): ``feed`` does the same through ``indices`` and ``index_select``."""

    def __init__(self, dataset_or_arrays, batch_size: int, device, seed: Optional[int] = None, rank: int = 0, world_size: int = 1):
        if hasattr(dataset_or_arrays, "particle_data"):
            particles, labels = dataset_or_arrays.particle_data, dataset_or_arrays.jet_features
        else:
            particles, labels = dataset_or_arrays
        particles = torch.as_tensor(particles, dtype=torch.float32)
        labels = torch.as_tensor(labels, dtype=torch.float32)
        if particles.dim() != 3 or particles.shape[-1] != 4 or particles.shape[0] < 1 or particles.shape[1] < 1:
            raise ValueError(f"expected normalised particles [n >= 1, N >= 1, 4], got {tuple(particles.shape)}")
        if labels.numel() != particles.shape[0]:
            raise ValueError(f"expected one label per jet, got {tuple(labels.shape)} for {particles.shape[0]} jets")
        if batch_size < 1 or world_size < 1 or not 0 <= rank < world_size:
            raise ValueError(f"batch_size {batch_size}, rank {rank} of {world_size}: not a slice of the stream")
        self.particle_data = particles.to(device).contiguous()
        self.device = self.particle_data.device     # (with its index: "cuda" is the current device)
        self.jet_features = labels.reshape(-1, 1).to(self.device).contiguous()
        self.n, self.num_particles = int(particles.shape[0]), int(particles.shape[1])
        self.batch_size, self.rank, self.world_size = int(batch_size), int(rank), int(world_size)
        s = torch.initial_seed() if seed is None else int(seed)
        self.key = (s * 0x9E3779B97F4A7C15 + LOADER_KEY_TERM) & 0xFFFFFFFFFFFFFFFF
        # the next stream position of this rank, in device memory: the feed launch reads it and moves it on (a replayed
        # hipGraph holds its address: it is written in place, never replaced)
        self.cursor = torch.full((1,), self.rank * self.batch_size, dtype=torch.int64, device=self.device)
        self._ticket = torch.zeros((1,), dtype=torch.int32, device=self.device)   # the launch's arrival counter: zero between launches
        self._base = 0    # the global position iteration 0 starts at (non-zero only behind a resume under another layout)
        self._captured = False   # (TrainStep: a captured feed launch holds the key as an argument)

    def __len__(self):
        return self.n

    @property
    def stride(self) -> int:
        return self.world_size * self.batch_size

    @property
    def steps_per_epoch(self) -> int:
        return -(-self.n // self.stride)

    @property
    def position(self) -> int:
        """This rank's next stream position (reads the cursor: synchronises)."""
        return int(self.cursor.item())

    @property
    def epoch(self) -> int:
        return self.position // self.n

    def indices(self, step: int) -> torch.Tensor:
        """The data-set rows of this rank's iteration ``step`` (0 = the first of the run) as a CPU int64 tensor, computed on
        the host by the kernel's own function (``mpg_shuffle_index_host``)."""
        from . import ops
        return ops.shuffle_indices(self.key, self._base + self.rank * self.batch_size + int(step) * self.stride, self.batch_size, self.n)

    def feed(self, step_buffers):
        """Write the next batch into ``step_buffers`` -- a ``TrainStep``, or anything with (some of) its attributes ``data``,
        ``labels``, ``_dcat``, ``_x3``, ``_mask2``, ``_ign2``, ``_labels2`` -- exactly as ``TrainStep.set_batch`` would, and move
        the cursor on: one launch on the current stream, capturable."""
        from . import ops
        B = self.batch_size
        buf = {k: getattr(step_buffers, a, None) for k, a in (("data", "data"), ("labels", "labels"), ("dcat", "_dcat"), ("x3", "_x3"),
                                                             ("mask2", "_mask2"), ("ign2", "_ign2"), ("labels2", "_labels2"))}
        if self.device.type == "cuda":
            ops.batch_feed(self.particle_data, self.jet_features, self.key, self.cursor, self._ticket, B, self.stride, **buf)
            return
        idx = ops.shuffle_indices(self.key, int(self.cursor.item()), B, self.n)
        x, l = self.particle_data.index_select(0, idx), self.jet_features.index_select(0, idx)
        for name, val in (("data", x), ("dcat", x), ("x3", x[..., :3]), ("mask2", x[..., 3:] + 0.5), ("ign2", 0.5 - x[..., 3]),
                          ("labels", l), ("labels2", torch.cat([l, l]))):
            t = buf[name]
            if t is not None:
                t[:val.shape[0]].copy_(val.reshape((val.shape[0],) + tuple(t.shape[1:])))
        self.cursor.add_(self.stride)

    def state_dict(self) -> dict:
        """The whole state of the data order (reads the cursor: synchronises)."""
        return {"key": self.key, "cursor": self.position, "n": self.n, "batch_size": self.batch_size, "rank": self.rank,
                "world_size": self.world_size}

    def load_state_dict(self, sd: dict):
        """Go on where the saved loader stopped.  The data set must be the one saved (same n).  Saved by another rank, or under
        another world or batch size: the cursor is re-derived from the GLOBAL position (where the saved step of all ranks
        began), so that the ranks of the resumed run consume the stream contiguously from there."""
        if int(sd["n"]) != self.n:
            raise ValueError(f"DeviceJetLoader: the saved state belongs to a data set of {int(sd['n'])} jets, this one has "
                             f"{self.n}: the shuffle is a permutation of the data set it was made for")
        key = int(sd["key"]) & 0xFFFFFFFFFFFFFFFF
        if self._captured and key != self.key:
            raise RuntimeError("DeviceJetLoader: the feed launch has been captured with this loader's key; load the saved state "
                               "before the first step")
        self.key = key
        glob = int(sd["cursor"]) - int(sd["rank"]) * int(sd["batch_size"])
        if glob < 0:
            raise ValueError(f"DeviceJetLoader: cursor {sd['cursor']} lies before rank {sd['rank']}'s first batch")
        self._base = glob % self.stride
        self.cursor.fill_(glob + self.rank * self.batch_size)
