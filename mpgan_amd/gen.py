"""Forward-only generation on the fused path -- the reference's ``gen`` / ``gen_multi_batch``
(train.py:100-282) and the un-normalising epilogue of its ``gen.py`` (:85-145).

Same function names and argument meaning as the reference, so ``train.py``'s evaluation loop and ``gen.py`` can call
these instead of their own; ``JetSampler`` is the bulk path built for the device (a captured chunk replayed over a keyed
stream of rows, labels drawn from the data set's multiplicities as gen.py:100-107 draws them).  Differences, all results-neutral: generation runs under ``torch.no_grad()`` whenever the
caller asked for detached output (the reference builds and then drops the autograd graph, train.py:253-282; without it
the fused MPLayer skips its sign words and saves nothing for a backward), and the default chunk is sized for the
device (thousands of jets per launch keep all 256 CUs busy; the reference's default of 16 leaves 240 idle).
"""
from __future__ import annotations

import logging
from typing import Optional

import torch
from torch import Tensor

from .data import FEATURE_MAXES, FEATURE_NORMS, FEATURE_SHIFTS, unnormalise_jets
from .mpgan.mask_utils import mask_manual


def get_gen_noise_shape(model_args: dict, num_samples: int, num_particles: int, model: str = "mpgan") -> tuple:
    """The shape of the generator's input noise per model family (train.py:100-140); see ``get_gen_noise``."""
    if model in ("mpgan", "old_mpgan"):
        if model_args.get("lfc"):
            return (num_samples, model_args["lfc_latent_size"])
        return (num_samples, num_particles + int(bool(model_args.get("mask_learn_sep"))), model_args["latent_node_size"])
    if model == "gapt":
        return (num_samples, num_particles, model_args["embed_dim"])
    if model == "rgan":
        return (num_samples, model_args["latent_dim"])
    raise NotImplementedError(f"mpgan_amd has a single noise shape for the mpgan, gapt and rgan model families only (got {model!r}; "
                              "treegan's noise is a list and pcgan has two noises: get_gen_noise)")


def get_gen_noise(model_args: dict, num_samples: int, num_particles: int, model: str = "mpgan", device=None,
                  noise_std: float = 0.2):
    """Generator input noise ~ N(0, noise_std) in the shape the model family takes (train.py:100-140):
    mpgan ``[n, N (+1 with mask_learn_sep), latent_node_size]`` (``[n, lfc_latent_size]`` with ``lfc``),
    gapt ``[n, N, embed_dim]``, rgan ``[n, latent_dim]`` (train.py:130-131), treegan the ONE-ELEMENT LIST
    ``[[n, 1, treegang_features[0]]]`` that ``ext_models.TreeGANG`` takes (train.py:132-133; a list has no single shape:
    ``get_gen_noise_shape`` declines it), pcgan ``[n, pcgan_latent_dim]`` for ``ext_models.latent_G`` (train.py:134-139),
    graphcnngan ``[n, latent_dim]`` for ``ext_models.GraphCNNGANG`` (train.py:130-131; no extra noise).
    Returns ``(noise, point_noise)`` like the reference: the second slot is None except for pcgan with
    ``model_args["sample_points"]``, where it is the decoder's per-particle noise ``[n, N, pcgan_z2_dim]`` ~ N(0, 1)."""
    if device is None:
        device = "cuda"
    if model == "pcgan":
        noise = torch.empty((num_samples, model_args["pcgan_latent_dim"]), device=device).normal_(0.0, noise_std)
        if not model_args["sample_points"]:
            return noise, None
        return noise, torch.empty((num_samples, num_particles, model_args["pcgan_z2_dim"]), device=device).normal_(0.0, 1.0)
    if model == "treegan":
        return [torch.empty((num_samples, 1, model_args["treegang_features"][0]), device=device).normal_(0.0, noise_std)], None
    if model == "graphcnngan":
        return torch.empty((num_samples, model_args["latent_dim"]), device=device).normal_(0.0, noise_std), None
    shape = get_gen_noise_shape(model_args, num_samples, num_particles, model)
    return torch.empty(shape, device=device).normal_(0.0, noise_std), None


def gen(model_args: dict, G: torch.nn.Module, num_samples: int, num_particles: int, model: str = "mpgan",
        noise: Tensor = None, labels: Tensor = None, noise_std: float = 0.2, **extra_args) -> Tensor:
    """``num_samples`` jets in one go (train.py:143-215): ``G(noise, labels)``, then the optional manual pT mask.  pcgan with
    ``model_args["sample_points"]``: the latent rows go through the decoder ``model_args["G_pc"]`` with per-particle noise
    (train.py:212-213); with a caller's ``noise`` that is ``extra_args["point_noise"]`` where given, else drawn here (the
    reference leaves it undefined there: a NameError)."""
    device = next(G.parameters()).device
    if labels is not None:
        assert labels.shape[0] == num_samples, "number of labels doesn't match num_samples"
        labels = labels.to(device)
    point_noise = extra_args.get("point_noise")
    if noise is None:
        noise, point_noise = get_gen_noise(model_args, num_samples, num_particles, model, device, noise_std)
    elif model == "pcgan" and model_args["sample_points"] and point_noise is None:
        _, point_noise = get_gen_noise(model_args, num_samples, num_particles, model, device, noise_std)
    gen_data = G(noise, labels)
    if extra_args.get("mask_manual"):
        gen_data = mask_manual(model_args, gen_data, extra_args["pt_cutoff"])
    if model == "pcgan" and model_args["sample_points"]:
        gen_data = model_args["G_pc"](gen_data.unsqueeze(1), point_noise)
    logging.debug(gen_data[0, :10])
    return gen_data


def gen_multi_batch(model_args: dict, G: torch.nn.Module, batch_size: int, num_samples: int, num_particles: int,
                    out_device: str = "cpu", detach: bool = False, use_tqdm: bool = True, model: str = "mpgan",
                    noise: Tensor = None, labels: Tensor = None, noise_std: float = 0.2, **extra_args) -> Tensor:
    """``num_samples`` jets in chunks of ``batch_size`` (train.py:226-282), gathered on ``out_device``.
    ``use_tqdm`` is accepted for signature compatibility (no progress bar is drawn)."""
    assert out_device == "cuda" or out_device == "cpu", "Invalid device type"
    if labels is not None:
        assert labels.shape[0] == num_samples, "number of labels doesn't match num_samples"
        labels = torch.as_tensor(labels, dtype=torch.float32)
    chunks = []
    with torch.set_grad_enabled(torch.is_grad_enabled() and not detach):
        for start in range(0, num_samples, batch_size):
            n = min(batch_size, num_samples - start)
            out = gen(model_args, G, num_samples=n, num_particles=num_particles, model=model, noise=noise,
                      labels=None if labels is None else labels[start:start + n], noise_std=noise_std, **extra_args)
            if detach:
                out = out.detach()
            chunks.append(out.to(out_device))
    return torch.cat(chunks, dim=0) if chunks else torch.empty(0)


def generate_jets(G: torch.nn.Module, num_samples: int, num_particles: int = 30, labels: Optional[Tensor] = None,
                  jet_type: str = "g", model: str = "mpgan", model_args: Optional[dict] = None, mask: bool = True,
                  batch_size: int = 4096, noise_std: float = 0.2) -> Tensor:
    """What the reference's ``gen.py`` writes to its output file: ``[num_samples, N, 3]`` un-normalised
    (eta_rel, phi_rel, pT_rel), masked particles zeroed (gen.py:111-141).  ``labels`` = num_particles / N per jet
    (gen.py samples them from the data set's jet features; the caller supplies them here)."""
    if model_args is None:
        model_args = ({"lfc": False, "latent_node_size": getattr(G, "input_node_size", 32)} if model == "mpgan"
                      else {"embed_dim": getattr(G, "embed_dim", 64)})
    was_training = G.training
    G.eval()
    try:
        jets = gen_multi_batch(model_args, G, batch_size, num_samples, num_particles, out_device="cuda", detach=True,
                               use_tqdm=False, model=model, labels=labels, noise_std=noise_std)
    finally:
        G.train(was_training)
    return unnormalise_jets(jets, jet_type, mask=mask)


SAMPLER_KEY_TERM = 0x8EBC6AF09C88C6E3   # tells a sampler's key from the loader's key and the device seed derived from the same torch seed


def sampler_key(seed: int) -> int:
    """The key of a ``JetSampler`` built with ``seed``: derived as ``DeviceJetLoader`` derives its own, with another term."""
    return (int(seed) * 0x9E3779B97F4A7C15 + SAMPLER_KEY_TERM) & 0xFFFFFFFFFFFFFFFF


def rank_chunks(num_samples: int, chunk: int, rank: int = 0, world: int = 1) -> list:
    """How a call for ``num_samples`` rows is dealt to rank ``rank`` of ``world`` that share one stream: the rows, counted from
    the call's first, of each of the rank's chunks, as half-open ranges in stream order.  The call consumes whole ROUNDS of
    ``world`` chunks -- ``ceil(ceil(num_samples / chunk) / world) * world`` -- and chunk c of the call goes to rank c mod world,
    so every rank gets the same number of ranges; a chunk at or beyond ``num_samples`` is an empty range, the one across it a
    short one.  Over the ranks the ranges partition [0, num_samples)."""
    num_samples, chunk, rank, world = int(num_samples), int(chunk), int(rank), int(world)
    if num_samples < 0 or chunk < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"rank_chunks: num_samples {num_samples} >= 0, chunk {chunk} >= 1 and 0 <= rank {rank} < world {world} expected")
    rounds = -(-(-(-num_samples // chunk)) // world)
    return [(min(c * chunk, num_samples), min((c + 1) * chunk, num_samples)) for c in range(rank, rounds * world, world)]


def _parts_ok(G) -> bool:
    """``G.generate_parts`` exists and takes this generator's options (it asserts mask_c without mask_feat_bin / use_mask)."""
    if not hasattr(G, "generate_parts"):
        return False
    ma = getattr(G, "mask_args", None)
    if ma is not None and (not ma.get("mask_c", True) or ma.get("mask_feat_bin", False)):
        return False
    return bool(getattr(G, "use_mask", True))


class JetSampler:
    """Bulk generation on the device: what the reference's ``gen.py`` does -- labels drawn from the data set's multiplicities
    (:100-107), ``G`` in chunks (:111-125), the un-normalising epilogue (:127-141) -- as ONE chunk of ``chunk`` jets that is
    captured once and replayed, with nothing drawn or sliced on the host.

    The output is a stream of rows g = 0, 1, 2, ... (include/mpgan_amd.h states it): row g's label is ``table[idx(g)]``, a keyed
    hash of the row alone (``ops.label_pick_indices`` recomputes it on the host); its noise is drawn under the seed word of its
    chunk c = g // chunk, ``ops.chunk_seed(key, c)``, at its place within the chunk.  Labels are a function of the row, noise of
    (chunk index, place in chunk): the same ``seed`` and ``chunk`` give the same jets whatever ran before.  ``sample`` always
    consumes whole chunks: a call for a number of jets that ``chunk`` does not divide leaves the rest of its last chunk's rows
    undelivered, and the next call goes on at the next chunk -- so two calls of 5 equal one call of 10 when ``chunk`` divides 5.

    One chunk is, on the current stream: ``ops.label_pick``; the noise and the rank mask in one launch under the sampler's own
    seed word; ``G.generate_parts`` under ``no_grad`` in eval mode; ``ops.jets_finish``, which writes the chunk's rows of the
    result and moves the cursor and the seed word on.  With ``use_graphs`` the first three are one hipGraph; ``jets_finish``
    stays outside it as the one eager launch per chunk, because the output array and its length are its arguments and differ
    from call to call (no recapture for a caller-owned ``out``).  A generator without ``generate_parts`` (or whose options it
    asserts against) runs as ``G(noise, labels)`` and ``jets_finish`` reads its [chunk, N, 4] rows in place.

    ``table``: a ``JetArrayDataset``, a ``DeviceJetLoader`` (their ``jet_features`` = num_particles / N) or a 1-D array of
    labels; kept on G's device.  ``seed`` (default ``torch.initial_seed()``) gives the key.  CUDA only (the product has no CPU
    path), ``chunk`` fixed for the sampler's life.

    ``rank`` / ``world_size`` / ``process_group``: data-parallel ranks built with the same ``seed``, ``chunk`` and table share the
    ONE stream above -- chunk c goes to rank c mod W (``rank_chunks``).  A call consumes whole rounds of W chunks, so every rank
    replays equally often; ``sample(n)`` returns this rank's rows of the next n in stream order, ``sample_all(n)`` -- a collective
    over ``process_group`` -- all n on every rank, bit for bit the rows a one-rank sampler gives while the ranks' weights are
    equal.  A rank's cursor starts at ``rank * chunk`` and ``jets_finish`` moves it by ``W * chunk``."""

    def __init__(self, G: torch.nn.Module, table, num_particles: int, jet_type: str = "g", chunk: int = 4096, model: str = "mpgan",
                 model_args: Optional[dict] = None, noise_std: float = 0.2, seed: Optional[int] = None, use_graphs: bool = True,
                 with_mask: bool = False, rank: int = 0, world_size: int = 1, process_group=None):
        from . import ops
        if isinstance(world_size, bool) or not isinstance(world_size, int) or world_size < 1 or not 0 <= int(rank) < world_size:
            raise ValueError(f"JetSampler: 0 <= rank < world_size expected, got rank = {rank!r}, world_size = {world_size!r}")
        self.rank, self.world, self.pg = int(rank), world_size, process_group
        dev = next(G.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError(f"JetSampler: the generator lives on {dev}; mpgan_amd has no CPU path (bulk generation runs on "
                               "the GPU: move the generator there)")
        if jet_type not in FEATURE_MAXES:
            raise ValueError(f"JetSampler: unknown jet type {jet_type!r} (one of {sorted(FEATURE_MAXES)})")
        if chunk < 1 or num_particles < 1:
            raise ValueError(f"JetSampler: chunk {chunk} x num_particles {num_particles} is not a chunk of jets")
        labels = table.jet_features if hasattr(table, "jet_features") else table
        self.table = torch.as_tensor(labels, dtype=torch.float32).reshape(-1).to(dev).contiguous()
        self.n = int(self.table.numel())
        if not 1 <= self.n <= 0x7FFFFFFF:
            raise ValueError(f"JetSampler: a table of 1 .. 2^31 - 1 labels expected, got {self.n}")
        if model_args is None:
            model_args = ({"lfc": False, "latent_node_size": getattr(G, "input_node_size", 32)} if model == "mpgan"
                          else {"embed_dim": getattr(G, "embed_dim", 64)})
        self.G, self.device, self.N, self.chunk, self.jet_type = G, dev, int(num_particles), int(chunk), jet_type
        self.noise_std, self.use_graphs, self.with_mask = float(noise_std), bool(use_graphs), bool(with_mask)
        self.key = sampler_key(torch.initial_seed() if seed is None else seed)
        B, N = self.chunk, self.N
        # the stream's state, in device memory: the launches read it and jets_finish moves it on (a replayed hipGraph holds
        # these addresses: they are written in place, never replaced)
        self.cursor = torch.full((1,), self.rank * B, dtype=torch.int64, device=dev)
        self.seed = torch.full((1,), ops.u64_as_i64(ops.chunk_seed(self.key, self.rank)), dtype=torch.int64, device=dev)
        self._ticket = torch.zeros((1,), dtype=torch.int32, device=dev)
        # the cursor as the host knows it (every chunk adds ``world * chunk``): what tells each launch where its rows go
        self._pos = self.rank * B
        self._stride = None if self.world == 1 else self.world * B      # (one rank: mpg_jets_finish as it was)
        # the chunk's static buffers
        noise_shape = get_gen_noise_shape(model_args, B, N, model)
        self.labels = torch.zeros((B, 1), device=dev)
        self.noise = torch.zeros(noise_shape, device=dev)
        self.mask = torch.zeros((B, N), device=dev)
        self.ignore = torch.zeros((B, N), device=dev)
        self.parts = _parts_ok(G)
        self.feat = torch.zeros((B, N, 3 if self.parts else 4), device=dev)
        self.premask = (self.parts and len(noise_shape) == 3 and noise_shape[1] == N and (N * noise_shape[2]) % 2 == 0
                        and getattr(G, "noise_mask_ok", lambda: False)())
        self._graph, self._graph_key = None, None

    # -- one chunk ------------------------------------------------------------------------------
    def _front(self):
        """Everything of a chunk in front of ``jets_finish``: labels, noise (+ masks), the generator.  Returns the mask
        [chunk, N] that ``jets_finish`` reads.  Reads the stream's state, moves nothing: the warm-up may run it freely."""
        from . import ops
        B, N = self.chunk, self.N
        ops.label_pick(self.table, self.key, self.cursor, B, self.labels)
        if self.premask:
            _, m, ig = ops.normal_noise_masked(tuple(self.noise.shape), self.noise_std, self.labels, device=self.device,
                                               mask_out=self.mask, ignore_out=self.ignore, seed_t=self.seed, out=self.noise)
            pm = (m, ig)
        else:
            ops.normal_noise(tuple(self.noise.shape), self.noise_std, device=self.device, seed_t=self.seed, out=self.noise)
            pm = None
        if self.parts:
            _, mask, _ = self.G.generate_parts(self.noise, self.labels, feat_out=self.feat, premask=pm,
                                               **({} if pm is not None else {"mask_out": self.mask}))
            if mask.data_ptr() != self.mask.data_ptr():
                self.mask.copy_(mask.reshape(B, N))
        else:
            self.feat.copy_(self.G(self.noise, self.labels))
            torch.add(self.feat[:, :, 3], 0.5, out=self.mask)
        return self.mask

    def _param_key(self):
        return tuple(p.data_ptr() for p in self.G.parameters())

    def _ensure_packed(self):
        """Weight images of the fused layers follow parameters that changed since the capture (an optimiser step,
        ``load_state_dict``): the check is the layers' own, made on the host in front of the replays."""
        for m in self.G.modules():
            if hasattr(m, "packed_sets"):
                for pk in m.packed_sets():
                    pk.ensure()

    def _capture(self, warmup: int = 2):
        """A short eager warm-up on a side stream (kernels loaded, ticket buffers and the allocator's pools filled -- none of
        which may happen during a capture), then the chunk's front as one hipGraph.  The warm-up reads the stream's state and
        moves none of it; every tensor that outlives the capture (the chunk buffers) was allocated when the sampler was built."""
        dev = self.device
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self._front()
        torch.cuda.current_stream(dev).wait_stream(s)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._front()
        self._graph, self._graph_key = g, self._param_key()

    # -- the public face ------------------------------------------------------------------------
    def sample(self, num_samples: int, out: Optional[Tensor] = None, mask_out: Optional[Tensor] = None):
        """The next ``num_samples`` jets of the stream, un-normalised ``[num_samples, N, 3]`` = (eta_rel, phi_rel, pT_rel)
        with masked particles zeroed -- what ``generate_jets`` returns --, plus their 0 / 1 masks ``[num_samples, N]`` when the
        sampler was built ``with_mask``.  ``out`` (``mask_out``): a caller-owned contiguous array of at least that many rows to
        write into (its first ``num_samples`` rows are returned).  A rank of several returns its own rows of those
        ``num_samples`` (``rank_chunks``), in stream order; every rank must make the call."""
        from . import ops
        total = int(num_samples)
        if total < 0:
            raise ValueError(f"sample: num_samples must be >= 0, got {total}")
        N, B, dev = self.N, self.chunk, self.device
        # this rank's chunks of the call: they land one behind the other in ``out`` -- full ones, then at most one short one,
        # then empty ones -- so the rank's row count is the ``total`` that every launch tests its rows against
        ranges = rank_chunks(total, B, self.rank, self.world)
        num_samples = sum(b - a for a, b in ranges)
        if out is not None and out.shape[0] == 0 and ranges and num_samples == 0:
            out = None       # (a rank without rows still runs its launches: they need an address)
        if out is None:
            out = torch.empty((max(num_samples, 1) if ranges else num_samples, N, 3), device=dev)
        if out.dim() != 3 or out.shape[0] < num_samples or tuple(out.shape[1:]) != (N, 3) or not out.is_contiguous() \
                or out.device != dev or out.dtype != torch.float32:
            raise ValueError(f"sample: out must be a contiguous float32 [>= {num_samples}, {N}, 3] tensor on {dev}, got {tuple(out.shape)}")
        if self.with_mask and mask_out is None:
            mask_out = torch.empty((num_samples, N), device=dev)
        if mask_out is not None and (mask_out.numel() < num_samples * N or not mask_out.is_contiguous() or mask_out.device != dev
                                     or mask_out.dtype != torch.float32):
            raise ValueError(f"sample: mask_out must be a contiguous float32 [>= {num_samples}, {N}] tensor on {dev}")
        was_training = self.G.training
        self.G.eval()
        try:
            with torch.no_grad():
                chunks = len(ranges)
                if chunks and self.use_graphs:
                    if self._graph is None or self._graph_key != self._param_key():
                        self._capture()
                    self._ensure_packed()
                for k in range(chunks):
                    if self.use_graphs:
                        self._graph.replay()
                        mask = self.mask
                    else:
                        mask = self._front()
                    ops.jets_finish(self.feat, mask, out, maxes=FEATURE_MAXES[self.jet_type], norms=FEATURE_NORMS,
                                    shifts=FEATURE_SHIFTS, key=self.key, cursor=self.cursor, seed=self.seed, ticket=self._ticket,
                                    row0=self._pos - k * B, total=num_samples, mask_out=mask_out, stride=self._stride)
                    self._pos += self.world * B
        finally:
            self.G.train(was_training)
        jets = out[:num_samples]
        return (jets, mask_out.reshape(-1, N)[:num_samples]) if self.with_mask else jets

    def _all_gather(self, t: Tensor) -> Tensor:
        """``t`` of every rank, [world, *t.shape] on the device.  RCCL gathers device memory; any other backend (gloo) gathers host
        copies -- the same bits either way."""
        import torch.distributed as dist
        src = t if dist.get_backend(self.pg) == "nccl" else t.cpu()
        parts = [torch.empty_like(src) for _ in range(self.world)]
        dist.all_gather(parts, src, group=self.pg)
        return torch.stack(parts).to(self.device)

    def sample_all(self, num_samples: int):
        """The next ``num_samples`` jets of the stream on EVERY rank, in stream order (and their masks ``with_mask``): each rank
        generates its own chunks (``sample``), one ``all_gather`` over ``process_group`` collects them and the chunks are
        interleaved back into the stream's order -- a collective, every rank calls it.  One rank: ``sample``."""
        if self.world == 1:
            return self.sample(num_samples)
        if self.pg is None:
            raise RuntimeError(f"sample_all: this sampler is rank {self.rank} of {self.world} without a process group to gather over")
        n, N, B = int(num_samples), self.N, self.chunk
        K = len(rank_chunks(n, B, self.rank, self.world))      # (chunks per rank: chunk k of this rank sits at rows k B ..)
        jets = torch.zeros((max(K * B, 1), N, 3), device=self.device)
        masks = torch.zeros((max(K * B, 1), N), device=self.device) if self.with_mask else None
        self.sample(n, out=jets, mask_out=masks)

        def in_stream_order(t):      # [W, K B, ...] -> rank r's chunk k is chunk k W + r of the call
            if K == 0:
                return t[:0]
            g = self._all_gather(t[:K * B]).reshape(self.world, K, B, *t.shape[1:])
            return g.transpose(0, 1).reshape(K * self.world * B, *t.shape[1:])[:n].contiguous()
        jets = in_stream_order(jets)
        return (jets, in_stream_order(masks)) if self.with_mask else jets

    @property
    def position(self) -> int:
        """The next stream row of this rank (reads the cursor: synchronises)."""
        return int(self.cursor.item())

    def state_dict(self) -> dict:
        """The whole state of the stream (reads the cursor: synchronises); a rank of several adds ``rank`` and ``world_size``."""
        sd = {"key": self.key, "cursor": self.position, "chunk": self.chunk, "n": self.n}
        if self.world > 1:
            sd.update(rank=self.rank, world_size=self.world)
        return sd

    def load_state_dict(self, sd: dict):
        """Go on where the saved sampler stopped.  The table must be the one saved (same n) and the chunk the same: the rows'
        labels are indices into that table, and their noise is cut into chunks of that size.  The state may come from another
        world size (any rank's): the saved GLOBAL position -- the rounds every saved rank had finished -- must then be a whole
        number of rounds of this sampler's world."""
        from . import ops
        if int(sd["n"]) != self.n:
            raise ValueError(f"JetSampler: the saved state belongs to a table of {int(sd['n'])} labels, this one has {self.n}")
        if int(sd["chunk"]) != self.chunk:
            raise ValueError(f"JetSampler: the saved state was cut into chunks of {int(sd['chunk'])} jets, this sampler's are {self.chunk}")
        cursor, saved_rank, saved_world = int(sd["cursor"]), int(sd.get("rank", 0)), int(sd.get("world_size", 1))
        if cursor < 0 or cursor % self.chunk:
            raise ValueError(f"JetSampler: cursor {cursor} is not a whole number of chunks of {self.chunk}")
        if saved_world < 1 or not 0 <= saved_rank < saved_world or cursor < saved_rank * self.chunk \
                or (cursor // self.chunk - saved_rank) % saved_world:
            raise ValueError(f"JetSampler: cursor {cursor} is not a position of rank {saved_rank} of {saved_world} at chunks of {self.chunk}")
        position = cursor - saved_rank * self.chunk      # the stream's row behind the last whole round of the saved world
        if position % (self.world * self.chunk):
            raise ValueError(f"JetSampler: the saved stream stands at row {position}, which is not a whole number of rounds of "
                             f"{self.world} chunks of {self.chunk}: this world of {self.world} cannot go on from there")
        cursor = position + self.rank * self.chunk
        key = int(sd["key"]) & 0xFFFFFFFFFFFFFFFF
        if key != self.key:       # (the key is an argument of the captured label_pick: capture again under the loaded one)
            self.key, self._graph = key, None
        self._pos = cursor
        self.cursor.fill_(cursor)
        self.seed.fill_(ops.u64_as_i64(ops.chunk_seed(self.key, cursor // self.chunk)))
