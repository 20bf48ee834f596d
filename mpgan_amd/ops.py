"""torch.autograd front-ends over the C ABI (include/mpgan_amd.h).

Everything here hands raw device pointers + sizes to libmpgan_amd.so on torch's current HIP
stream; torch is used for memory, autograd bookkeeping and a few tiny reductions only.  There is
no CPU path: tensors must live on a gfx950 device.  (One exception, for checking a derivative rule in fp64 without a GPU:
``EdgeRowsFn`` / ``EdgeRowsVJPFn``, ``AttnCoreFn``, ``LinearNetFn`` and ``DiscHeadDDFn`` evaluate CPU tensors with the same formulas in
plain torch.)
"""
from __future__ import annotations

import contextlib
import ctypes as C
import itertools
import os
import sys
import threading
from collections import namedtuple
from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import MpgGemm, MpgEdgeFwd, MpgEdgeBwd, MpgEdgeDw, MpgKnnEdgeFwd, MpgKnnEdgeBwd, MpgKnnEdgeJvp, MpgPackJob, MpgChain, MpgReduceJob, check

H1, H2, H3 = 96, 160, 192
# Exact power-of-two operand scales of the forward products (csrc/edge_common.h): fp16 hi/lo pairs keep their 22 bits
# only for |x| >= 2^-3, so the forward images hold SC * W and the activations are split as ascale * x.
SC_W2, SC_W3 = 16.0, 64.0          # = SC_W2 / SC_W3 of csrc/edge_common.h
SC_WN, SC_ACT = 64.0, 8.0          # node-network (mpg_chain) images / activations
TAG_E0, TAG_E1, TAG_E2, TAG_N0, TAG_N1, TAG_N2, TAG_GENERIC = 1, 2, 3, 4, 5, 6, 7

# ------------------------------------------------------------------------------------- state
# Read-only configuration of the arithmetic (set before building models; not step state).
OPTIONS = {
    "skip_masked": True,      # edge forward: skip zero-masked senders (they contribute exactly 0)
    # launches with more workgroups than CUs (the discriminator's real + generated batch) hand their jets out heaviest first
    # (mpg_jet_order): no effect on results, 136 -> 113 us on the 2B launches of the headline configuration
    "lpt_order": True,
    # the node network fn as the epilogue of the fused edge forward (mpg_edge_fwd_fn: one launch instead of two, same bits);
    # False = mpg_edge_fwd followed by mpg_chain
    "fn_epilogue": os.environ.get("MPG_FN_EPILOGUE", "1") != "0",
    # ... and, in the backward, the layer's dx chain and the layer-below's node-network input-gradient chain as the epilogue of the
    # data-gradient kernel (mpg_edge_bwd_fn: one launch instead of three); False = mpg_edge_bwd followed by the mpg_chain calls
    "bwd_epilogue": os.environ.get("MPG_BWD_EPILOGUE", "1") != "0",
    # sender-chunked launches (N > 32 on few jets: SC > 1) keep the node network as the edge forward's epilogue too: the workgroup of
    # a (jet, receiver block) that arrives LAST adds up the chunks' partial sums (mpg_edge_fwd_fn with MpgEdgeFwd.tickets); False =
    # mpg_edge_fwd, a sum over the chunk axis and the mpg_chain calls
    "fn_chunks": os.environ.get("MPG_FN_CHUNKS", "1") != "0",
    # the per-workgroup reduction of mpg_edge_dw inside the layer's grouped split-K reduction launch (mpg_splitk_reduce_group_dw)
    "dw_reduce_grouped": os.environ.get("MPG_DW_REDUCE_GROUPED", "1") != "0",
    # product form of the fused edge forward (MpgEdgeFwd.two_term): 0 = three 16-bit terms in every product; 1 = fe.net.2 on two terms
    # (its input E2 as the one fp16 value that is parked for the backward anyway): -15 % per launch, pre-activations of fe.net.2 to
    # ~1e-4 of their scale instead of ~5e-7.  MPG_FWD_TWO_TERM.
    "fwd_two_term": int(os.environ.get("MPG_FWD_TWO_TERM", "0")),
    # spectral-norm networks: the normalised weights of all wrapped layers of a LinearNet / an MPLayer from ONE grouped launch
    # (mpg_spectral_norm) and such MPLayers on the fused edge kernels; False = a launch per wrapped layer and MPLayer._forward_edges
    "sn_fused": os.environ.get("MPG_SN_FUSED", "1") != "0",
    # fused MPLayers on a k-nearest-neighbour graph (fully_connected=False) on the SPARSE edge kernels (mpg_knn_edge_fwd / _bwd: the
    # B * N * k rows of the neighbour sets) instead of the dense kernels with the neighbour bit as a factor over all N * N pairs;
    # see ``knn_sparse_route`` for what it covers.  Off unless asked for: MPG_KNN_SPARSE=1.
    "knn_sparse": os.environ.get("MPG_KNN_SPARSE", "0") not in ("", "0"),
    # the gradient penalty's edge aggregation on the row kernels (``EdgeRowsFn``: mpg_knn_edge_fwd / _bwd / _jvp, twice differentiable)
    # instead of the materialised edge matrix of MPLayer._forward_edges, for the layers ``gp_rows_route`` covers.  Off unless asked
    # for: MPG_GP_ROWS=1, or TrainStep(gp_rows=True).
    "gp_rows": os.environ.get("MPG_GP_ROWS", "0") not in ("", "0"),
    # the gradient penalty's attention core (softmax(q k^T / sqrt(d)) v of every MAB) on the attention kernels (``AttnCoreFn``:
    # mpg_attn_fwd / _bwd / _dd, twice differentiable) instead of the broadcast products of MAB._forward_dd, for the blocks
    # ``gp_attn_route`` covers.  Off unless asked for: MPG_GP_ATTN=1, or TrainStep(gp_attn=True).
    "gp_attn": os.environ.get("MPG_GP_ATTN", "0") not in ("", "0"),
    # the gradient penalty's LinearNets as one twice-differentiable op each (``LinearNetFn``: mpg_chain for the forward, the
    # input-gradient chain and the tangent chain, one grouped launch for all weight gradients, keyed dropout) instead of the
    # MatMulFn / bias / leaky_relu / dropout composites of LinearNet._forward_dd, for the nets ``gp_chain_route`` covers, and the
    # discriminator's pooling + fnd_layer + sigmoid on ``DiscHeadDDFn`` (mpg_disc_head_fwd / _dd).  Off unless asked for:
    # MPG_GP_CHAIN=1, or TrainStep(gp_chain=True).
    "gp_chain": os.environ.get("MPG_GP_CHAIN", "0") not in ("", "0"),
    # the set-pooling baselines (ext_models.rGAND / PointNetMixD): the last per-particle layer and the max / mean over a jet's
    # particles as one launch (``PointPoolFn``: mpg_point_pool_fwd / _bwd) for the shapes ``point_pool_route`` covers; False
    # (MPG_POINT_POOL=0) = ``FusedLinearFn`` for the layer, then torch.max / torch.mean on its [B N, C] output
    "point_pool": os.environ.get("MPG_POINT_POOL", "1") != "0",
    # the TreeGAN generator (ext_models.TreeGANG): a TreeGCN layer as one launch per direction (``TreeGcnFn``: mpg_tree_gcn_fwd /
    # _bwd, W_loop collapsed to one [out, in] matrix) for the shapes ``tree_gcn_route`` covers; False (MPG_TREE_GCN=0) = the
    # reference's literal layer on ``FusedLinearFn``, torch.matmul and ATen's LeakyReLU, its [rows, in support] activation included
    "tree_gcn": os.environ.get("MPG_TREE_GCN", "1") != "0",
    # PCGAN's set encoder (ext_models.G_inv_Tanh / G_inv): the equivariant stack ``phi`` and the max over a jet's particles as one
    # forward-only launch (``set_encode_launch``: mpg_set_encode_fwd, the [B N, d_dim] activations stay in LDS) where
    # ``set_encode_route`` says yes; False (MPG_SET_ENCODE=0) = layer by layer on ``FusedLinearFn`` and ATen's max / mean / tanh /
    # softplus, which is also the differentiable route
    "set_encode": os.environ.get("MPG_SET_ENCODE", "1") != "0",
    # the GraphCNN-GAN generator (ext_models.GraphCNNGANG): an NNConv layer (mean aggregation, root weight, bias) as one launch per
    # direction (``NNConvFn``: mpg_nnconv_fwd / _bwd, the factorised form [P | m | x] [W3 ; Bn ; root]: no weight matrix per edge)
    # for the shapes ``nnconv_route`` covers; False (MPG_NNCONV=0) = the literal layer: gather, a [B N k, Cin Cout] per-edge weight
    # tensor from ``FusedLinearFn``, torch.bmm, the mean over the listed neighbours
    "nnconv": os.environ.get("MPG_NNCONV", "1") != "0",
}
NUM_CUS = 256
# Forward products (they decide LeakyReLU signs) are split as fp16 hi/lo with the operand scales below (~2^-21 per
# product); the fused edge backward works in fp16 as well (csrc/edge_bwd2_impl.h).  Range: |e2| < 1023, node activations
# < 8188, |W * dscale| < 1023 -- see INTEGRATION.md.  ``mpg_gemm`` (``linear_fwd``) has no operand scales: its fp16 route holds
# 1e-4 (TIGHT) for operand magnitudes down to about 2^-10 and 1e-3 (TOL) down to about 2^-16; below that the product fades
# out, above 65504 it is inf.  The bf16 route has no such range (tests/split_ref.py).
FWD_F16 = True


class DeviceState:
    """Everything mutable the fused ops keep between calls, ONE INSTANCE PER DEVICE (SURVEY.md section 8b:
    the reference's ``nn.DataParallel`` drives each device from its own thread, and autograd runs a device's
    backward nodes on that device's worker thread -- so the key is the device, not the calling thread).

    seed            64-bit dropout seed in device memory (a captured hipGraph sees a new value on every replay)
    tags / last_tag dropout-site tag counter of fused-op invocations on this device
    grad_into_param ``FusedMPLayerFn.backward`` adds parameter gradients straight into ``param.grad`` and returns
                    None for them (``train.TrainStep`` switches it on around its backward; leave it off when
                    ``torch.autograd.grad``, hooks or anything else needs the gradients as autograd values)
    deferred_wgrad  a ``WgradBatch`` that collects the stand-alone Linear layers' weight gradients of the
                    backward in flight (``TrainStep`` flushes it as grouped launches), or None
    wgrad_stream    a second stream for the launches that only produce WEIGHT gradients (``mpg_edge_dw`` + its reduction, the
                    grouped node-network weight gradients): nothing reads them before the optimizer, so ``FusedMPLayerFn.backward``
                    forks them off behind ``mpg_edge_bwd`` and goes on with the data gradients; ``TrainStep`` sets it around a
                    backward and joins before the optimizer step / all-reduce.  ``wgrad_keep`` holds every tensor those
                    launches touch until the join (the allocator must not hand their memory to main-stream work meanwhile)
    double_backward modules built while it is set (``double_backward_route``) take the route whose backward is itself
                    differentiable: the gradient penalty's ``torch.autograd.grad(..., create_graph=True)`` (train.py:304-311)
    """

    def __init__(self, index: int):
        self.index = index
        self._seed = None
        self.seed_is_default = True   # nobody has called set_seed on this device yet (TrainStep then seeds it itself)
        self.auto_seed_key = None     # (torch seed, rank) TrainStep last seeded this device from: a second TrainStep under the same pair leaves the stream where it is
        self.tags = itertools.count(1)
        self.last_tag = 0
        self.tag_log = None
        self.sign_tap = None   # tests: a list that collects, per fused MPLayer call with a backward, the tensors its kink decisions can be read from
        self.grad_into_param = False
        self.deferred_wgrad = None
        self.wgrad_stream = None
        self.wgrad_keep = []
        self.double_backward = False
        self._status = None

    @property
    def status(self) -> torch.Tensor:
        """Range guard of the packed weight images: a device word ``mpg_pack_many`` ORs into (1: an fp16 image element beyond
        65504 after scaling, 2: a non-finite weight).  ``range_status`` reads it."""
        if self._status is None:
            dev = torch.device("cuda", self.index) if self.index >= 0 else torch.device("cpu")
            self._status = torch.zeros((1,), dtype=torch.int32, device=dev)
        return self._status

    @property
    def seed(self) -> torch.Tensor:
        if self._seed is None:  # created on first use: the host-side state exists without touching the device
            dev = torch.device("cuda", self.index) if self.index >= 0 else torch.device("cpu")
            self._seed = torch.full((1,), 0x243F6A8885A308D3, dtype=torch.int64, device=dev)
        return self._seed


_states = {}
_states_lock = threading.Lock()


def _dev_index(device) -> int:
    """Device ordinal of ``device`` (a torch.device, a string or an int); a bare "cuda" means the CURRENT device,
    not device 0.  CPU (host-logic tests of ``train.TrainStep`` with toy modules) maps to -1."""
    if isinstance(device, int):
        return device
    d = torch.device(device)
    if d.type == "cpu":
        return -1
    if d.index is not None:
        return d.index
    return torch.cuda.current_device() if torch.cuda.is_available() else 0


def dev_state(device) -> DeviceState:
    idx = _dev_index(device)
    st = _states.get(idx)
    if st is None:
        with _states_lock:
            st = _states.get(idx)
            if st is None:
                st = _states[idx] = DeviceState(idx)
    return st


def seed_tensor(device) -> torch.Tensor:
    """Per-device 64-bit dropout seed living in device memory.  ``bump_seed`` advances it; call once per
    training iteration."""
    return dev_state(device).seed


def range_status(device="cuda", clear: bool = False) -> int:
    """What the range guard has seen on ``device`` since it was last cleared (0 = nothing; synchronises): bit 0 = a weight times
    its operand scale left fp16's range while the images were packed (the fused forward then multiplies with inf), bit 1 =
    a weight was not finite."""
    st = dev_state(device).status
    v = int(st.item())
    if clear:
        st.zero_()
    return v


def set_seed(value: int, device="cuda", _auto: bool = False):
    """Set the device-resident 64-bit seed that keys every counter-based stream of the fused path on ``device``: the dropout
    masks and -- inside ``train.TrainStep`` -- the generator's input noise.  ``torch.manual_seed`` does NOT reach these
    streams.  ``TrainStep`` seeds a device nobody has seeded from ``torch.initial_seed()`` and its rank (so that
    ``torch.manual_seed(seed)`` keeps the reference's meaning, setup_training.py:184, and ranks draw different noise and
    masks); call this after constructing it to choose the value yourself, with a different value on every rank
    (``dist.rank_seed``)."""
    v = int(value) & 0xFFFFFFFFFFFFFFFF          # the 64-bit pattern as the kernels read it (an int64 tensor holds it signed)
    seed_tensor(device).fill_(v - (1 << 64) if v >= (1 << 63) else v)
    st = dev_state(device)
    st.seed_is_default = _auto   # (TrainStep's own choice does not count as the caller's)
    if not _auto:
        st.auto_seed_key = None


def derived_seed(torch_seed: int, rank: int) -> int:
    """The device seed ``TrainStep`` derives from torch's seed and the data-parallel rank: distinct per (seed, rank)."""
    return (torch_seed * 0x9E3779B97F4A7C15 + (rank + 1) * 0xD1B54A32D192ED03 + 0x243F6A8885A308D3) & 0x7FFFFFFFFFFFFFFF


RANK_TERM = 0xD1B54A32D192ED03   # what one step in rank adds to ``derived_seed``


def rerank_seed(saved: int, saved_rank: int, rank: int) -> int:
    """The seed a checkpoint written by rank ``saved_rank`` hands to rank ``rank``: the saved value moved by the rank term of
    ``derived_seed`` once per rank of distance (mod 2^64).  The reference keeps ONE ``G_optim_<epoch>.pt`` per epoch
    (train.py:534-535), written by one process: loaded as it is, every rank of a resumed data-parallel run would draw rank 0's
    noise and dropout masks from there on.  The saving rank itself gets the saved value back bit for bit (resume == uninterrupted
    run); the others get streams of their own, distinct for every rank."""
    return (int(saved) + (int(rank) - int(saved_rank)) * RANK_TERM) & 0xFFFFFFFFFFFFFFFF


def get_seed(device="cuda") -> int:
    """The seed's current value as an unsigned 64-bit number (synchronises; checkpoints)."""
    return int(seed_tensor(device).item()) & 0xFFFFFFFFFFFFFFFF


SEED_STEP = 0x1E3779B97F4A7C15   # what an iteration adds to the seed


def bump_seed(device="cuda"):
    seed_tensor(device).add_(SEED_STEP)


# The tag table of include/mpgan_amd.h (MPG_*_TAG; a family's tags are its base + a site or round number): disjoint spans above
# the dropout sites' tags, which ``next_tag`` keeps below 2^27 (csrc/draws.h asserts it; tests/test_cabi_cpu.py compares the two)
NOISE_TAG = 0x4E000000     # ``normal_noise``: + site
AUG_TAG = 0x41000000       # ``augment``: + site
LABEL_TAG = 0x4C000000     # ``label_targets``: + site
SHUFFLE_TAG = 0x53000000   # the keyed shuffle: + Feistel round
PICK_TAG = 0x50000000      # ``label_pick``


def _noise_target(shape, device, out):
    if out is None:
        return torch.empty(shape, device=device, dtype=torch.float32)
    _chk(out, "out")
    if tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError(f"noise: out must be a contiguous tensor of shape {tuple(shape)}, got {tuple(out.shape)}")
    return out


def normal_noise(shape, std: float, site: int = 0, device="cuda", mean: float = 0.0, seed_t: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A fresh [*shape] tensor of N(mean, std^2) samples from the counter-based stream of ``mpg_normal``: keyed by the
    device's seed (``bump_seed`` once per iteration) and ``site`` (which draw of the iteration).  The generator's input noise
    (train.py:100-141) inside a captured iteration: no torch generator state to carry through the graph.
    ``seed_t``: another 64-bit seed word in device memory (one int64; ``gen.JetSampler`` keys its chunks with its own) instead
    of the device's; ``out``: the tensor to write into."""
    out = _noise_target(shape, device, out)
    seed_t = _seed_word(seed_t, out.device)
    check(_lib.lib().mpg_normal(_p(out), out.numel(), _p(seed_t), NOISE_TAG + int(site), mean, std, _stream()), "mpg_normal")
    return out


def _seed_word(seed_t: Optional[torch.Tensor], device) -> torch.Tensor:
    """The seed word a noise launch reads: the caller's (one int64 on ``device``) or the device's own."""
    if seed_t is None:
        return seed_tensor(device)
    if seed_t.dtype != torch.int64 or seed_t.numel() != 1 or seed_t.device != device:
        raise ValueError(f"seed_t: one int64 on {device} expected, got {seed_t.dtype} {tuple(seed_t.shape)} on {seed_t.device}")
    return seed_t


def next_tag(device="cuda", kind: str = "", thr: int = 0) -> int:
    """A fresh dropout-site tag base (8 sites per call) for one fused-op invocation on ``device``.  ``kind`` / ``thr`` name the
    invocation in ``DeviceState.tag_log`` (tests: a list there collects (kind, tag base, thr) of every invocation, in host
    order, so that a whole iteration's keep masks can be dumped site by site with ``dropout_mask``)."""
    st = dev_state(device)
    st.last_tag = (next(st.tags) % (1 << 24)) * 8
    if st.tag_log is not None:
        st.tag_log.append((kind, st.last_tag, int(thr)))
    return st.last_tag


def last_tag(device="cuda") -> int:
    """Tag base of the most recent fused-op invocation on ``device`` (tests: dump that call's dropout masks)."""
    return dev_state(device).last_tag


def drop_params(p: float):
    """thr = round(256 p) (keep <=> byte >= thr); scale = 256/(256-thr)."""
    thr = int(round(256.0 * p))
    if thr <= 0:
        return 0, 1.0
    if thr >= 256:
        raise ValueError("dropout p too close to 1")
    return thr, 256.0 / (256.0 - thr)


TICKET_SLOTS = 32


def _tickets(device, n: int) -> torch.Tensor:
    """Arrival counters for ONE launch whose workgroups hand a reduction to the last arriver: ``n`` zeros that the launch leaves
    zero.  Every call gets the next of ``TICKET_SLOTS`` regions of a per-device buffer: launches that run side by side on two
    streams (the generator-ahead branch beside the D step's own generator call) must not count on the same words, and a
    captured launch keeps the region it was given.  A buffer that has been handed out is NEVER freed (a replayed hipGraph keeps
    raw pointers into it: a larger request gets a new buffer, the old one stays on ``DeviceState``), and a new buffer is zeroed
    and the device synchronised before its first region goes out, whichever stream asks first (``TrainStep`` reserves it for its
    largest launch when it is built)."""
    buf = reserve_tickets(device, n)
    st = dev_state(device)
    st._ticket_i = (st._ticket_i + 1) % TICKET_SLOTS
    return buf[st._ticket_i]


def reserve_tickets(device, n: int) -> torch.Tensor:
    """Make sure the device's ticket buffer has regions of at least ``n`` words (``TrainStep`` calls this when it is built, for its
    largest launch: a capture with ``warmup=0`` then finds the buffer ready)."""
    st = dev_state(device)
    buf = getattr(st, "_tickets", None)
    per = max(4096, n)
    if buf is None or buf.shape[1] < per:
        if buf is not None:
            st._tickets_retired = getattr(st, "_tickets_retired", []) + [buf]
        buf = torch.zeros((TICKET_SLOTS, per), dtype=torch.int32, device=device)
        # the zeros are there for every stream (the launches that use them run on several).  Inside a capture -- a module captured
        # without a TrainStep in front of it -- the fill is a node of that graph, ordered before the captured launches.
        if not torch.cuda.is_current_stream_capturing():
            torch.cuda.synchronize(device)
        st._tickets, st._ticket_i = buf, 0
    return buf


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[torch.Tensor], offset_elems: int = 0):
    if t is None:
        return None
    return C.c_void_p(t.data_ptr() + 4 * offset_elems)


def _chk(t: torch.Tensor, name: str):
    if not (t.is_cuda and t.dtype == torch.float32):
        raise RuntimeError(f"{name}: expected a float32 tensor on the GPU (got {t.dtype} on {t.device}); "
                           "mpgan_amd has no CPU path")


# ------------------------------------------------------------------------------------- GEMM
def gemm(A, lda, B, ldb, Cout, ldc, M, N, K, *, ak=True, bk=True, a_off=0, b_off=0, c_off=0,
         A2=None, lda2=0, K1=0, bias=None, out_scale=1.0, act=False, alpha=0.2,
         drop=None, gate=None, resid=None, ldr=0, accumulate=False, splitk=1, split_stride=0, f16=False,
         ones_col=False):
    """Thin wrapper of mpg_gemm.  drop = (seed_t, tag, thr, scale) applies forward dropout to C;
    gate = (H, ldh, gate_act, seed_t, tag, thr, scale) multiplies C by d(dropout o act)/dz."""
    g = MpgGemm()
    g.A, g.A2, g.lda, g.lda2, g.K1 = _p(A, a_off), _p(A2), lda, lda2, K1
    g.B, g.ldb = _p(B, b_off), ldb
    g.C, g.ldc = _p(Cout, c_off), ldc
    g.M, g.N, g.K = M, N, K
    g.split_stride = split_stride
    g.bias, g.out_scale, g.act, g.alpha = _p(bias), out_scale, int(act), alpha
    g.seed = None
    if drop is not None and drop[2]:
        g.seed = _p(drop[0]); g.drop_tag, g.drop_thr, g.drop_scale = drop[1], drop[2], drop[3]
    if gate is not None:
        H, ldh, gact, seed_t, tag, thr, scale = gate
        g.gateH, g.ldh, g.gate_act = _p(H), ldh, int(gact)
        if thr:
            g.seed = _p(seed_t); g.gate_tag, g.gate_thr, g.gate_scale = tag, thr, scale
    g.resid, g.ldr = _p(resid), ldr
    g.accumulate = int(accumulate)
    g.f16 = int(f16)
    g.ones_col = int(ones_col)
    check(_lib.lib().mpg_gemm(C.byref(g), int(ak), int(bk), splitk, _stream()), "mpg_gemm")


def linear_fwd(x, W, bias=None, *, act=False, alpha=0.2, drop=None, x2=None, w_col0=0, w_cols=None, resid=None, f16=None):
    """y = drop(act([x | x2] @ W[:, w_col0:w_col0+K]^T + bias)) (+ resid).  x [M,K1], W [N,ldw].  ``f16``: fp16 hi/lo
    operands (the forward's default: ~2^-21 per product at unit magnitude) or bf16 hi/lo (~2^-17, any magnitude).  The fp16 route
    carries no operand scales: it holds 1e-4 (TIGHT) for operand magnitudes down to about 2^-10 and 1e-3 (TOL) down to about
    2^-16; below that the product fades out, and above 65504 it is inf.  The bf16 route has no such range."""
    M, K1 = x.shape
    K2 = 0 if x2 is None else x2.shape[1]
    K = K1 + K2 if w_cols is None else w_cols
    N = W.shape[0]
    y = torch.empty((M, N), device=x.device, dtype=torch.float32)
    gemm(x, x.stride(0), W, W.stride(0), y, N, M, N, K, ak=True, bk=True, b_off=w_col0,
         A2=x2, lda2=0 if x2 is None else x2.stride(0), K1=K1, bias=bias, act=act, alpha=alpha, drop=drop,
         resid=resid, ldr=0 if resid is None else resid.stride(0), f16=FWD_F16 if f16 is None else f16)
    return y


def linear_bwd_data(dy, W, *, w_col0=0, w_cols=None, gate=None, out=None, accumulate=False, alpha=0.2):
    """dx = (dy @ W[:, w_col0:w_col0+K]) * gate.   dy [M,N], W [N,ldw] -> dx [M,K]."""
    M, N = dy.shape
    K = (W.shape[1] - w_col0) if w_cols is None else w_cols
    if out is None:
        out = torch.empty((M, K), device=dy.device, dtype=torch.float32)
    gemm(dy, dy.stride(0), W, W.stride(0), out, out.stride(0), M, K, N, ak=True, bk=False, b_off=w_col0,
         gate=gate, accumulate=accumulate, alpha=alpha)
    return out


def linear_bwd_weight(dy, x, *, out=None, out_col0=0, out_scale=1.0, bias_out=None):
    """dW[:, out_col0:out_col0+K] = out_scale * dy^T @ x  (dy [M,N], x [M,K]; split-K over M), and, when
    ``bias_out`` [N] is given, bias_out = column sums of dy (a virtual ones column of x, same launch)."""
    M, N = dy.shape
    K = x.shape[1]
    if out is None:
        out = torch.empty((N, K), device=dy.device, dtype=torch.float32)
    hb = int(bias_out is not None)
    tiles = ((N + 63) // 64) * ((K + hb + 63) // 64)
    splitk = max(1, min((M + 255) // 256, (1024 + tiles - 1) // tiles))
    part = torch.empty((splitk, N, K + hb), device=dy.device, dtype=torch.float32)
    gemm(dy, dy.stride(0), x, x.stride(0), part, K + hb, N, K + hb, M, ak=False, bk=False, out_scale=out_scale,
         splitk=splitk, split_stride=N * (K + hb), ones_col=bool(hb))
    check(_lib.lib().mpg_splitk_reduce(_p(part), splitk, N, K, hb, _p(out, out_col0), out.stride(0), _p(bias_out),
                                       _stream()), "mpg_splitk_reduce")
    return out


# (train.TrainStep sets DeviceState.deferred_wgrad around a backward: FusedLinearFn then queues its weight gradients
# there instead of launching one small split-K GEMM + reduction per layer; TrainStep flushes the queue -- grouped
# launches -- before the optimizer.)
# workgroups a single weight-gradient GEMM of a group aims for when choosing its split-K factor
WGRAD_TARGET_WGS = int(os.environ.get("MPG_WGRAD_TARGET", "512"))


GROUP_MAX = 16   # MPG_GROUP_MAX of include/mpgan_amd.h


class WgradBatch:
    """Weight gradients dW[:, col0:col0+K] = scale * dy^T @ x (+ bias = column sums of dy) collected and issued as
    ONE grouped split-K GEMM launch plus ONE grouped reduction (``linear_bwd_weight`` does one at a time)."""

    def __init__(self):
        self.jobs = []

    def add(self, dy, x, *, out, out_col0=0, out_scale=1.0, bias_out=None, accumulate=False):
        M, N = dy.shape
        K = x.shape[1]
        hb = int(bias_out is not None)
        # (a ones column that would sit alone in a tile column of its own -- K a multiple of 64 -- is folded into the
        # workgroups of tile column 0 by the kernel: csrc/gemm.hip)
        kcols = K if (hb and K % 64 == 0) else K + hb
        tiles = ((N + 63) // 64) * ((kcols + 63) // 64)
        splitk = max(1, min((M + 255) // 256, (WGRAD_TARGET_WGS + tiles - 1) // tiles))
        part = torch.empty((splitk, N, K + hb), device=dy.device, dtype=torch.float32)
        self.jobs.append((dy, x, out, out_col0, out_scale, bias_out, splitk, part, accumulate))

    def _groups(self):
        """The queue cut into launches: at most GROUP_MAX jobs each, in order, and no two jobs of a launch writing the same buffer
        -- the grouped reduction adds into ``out`` / ``bias_out`` with a plain read and write per element, so two jobs of ONE
        launch on the same target (a module applied twice in one backward: D's two passes of ``batch_real_fake=False``) would
        lose one of the two sums; in launches of their own they are ordered by the stream."""
        groups, cur, seen = [], [], set()
        for job in self.jobs:
            out, col0, bias_out = job[2], job[3], job[5]
            targets = {(out.data_ptr(), col0)} | (set() if bias_out is None else {(bias_out.data_ptr(), 0)})
            if len(cur) == GROUP_MAX or targets & seen:
                groups.append(cur)
                cur, seen = [], set()
            cur.append(job)
            seen |= targets
        return groups + ([cur] if cur else [])

    def flush(self, dw=None):
        """``dw``: an ``MpgEdgeDw`` whose launch ran with ``defer_reduce`` -- its per-workgroup reduction rides in the first group's
        reduction launch (``mpg_splitk_reduce_group_dw``; with no job at all it is that launch alone)."""
        if dw is not None and not self.jobs:
            check(_lib.lib().mpg_splitk_reduce_group_dw(None, 0, C.byref(dw), _stream()), "mpg_splitk_reduce_group_dw")
        for i0, jobs in enumerate(self._groups()):
            n = len(jobs)
            gs, sk, rj = (MpgGemm * n)(), (C.c_int * n)(), (MpgReduceJob * n)()
            for i, (dy, x, out, col0, scale, bias_out, splitk, part, acc) in enumerate(jobs):
                M, N = dy.shape
                K = x.shape[1]
                hb = int(bias_out is not None)
                g = gs[i]
                g.A, g.lda, g.B, g.ldb = _p(dy), dy.stride(0), _p(x), x.stride(0)
                g.C, g.ldc = _p(part), K + hb
                g.M, g.N, g.K = N, K + hb, M
                g.split_stride, g.out_scale, g.alpha, g.ones_col = N * (K + hb), scale, 0.2, hb
                sk[i] = splitk
                r = rj[i]
                r.part, r.S, r.N, r.K, r.has_bias = _p(part), splitk, N, K, hb
                r.out, r.ldo, r.bias, r.accumulate = _p(out, col0), out.stride(0), _p(bias_out), int(acc)
            check(_lib.lib().mpg_gemm_wgrad_group(gs, sk, n, _stream()), "mpg_gemm_wgrad_group")
            if dw is not None and i0 == 0:
                check(_lib.lib().mpg_splitk_reduce_group_dw(rj, n, C.byref(dw), _stream()), "mpg_splitk_reduce_group_dw")
            else:
                check(_lib.lib().mpg_splitk_reduce_group(rj, n, _stream()), "mpg_splitk_reduce_group")
        self.jobs = []


def gate(g, H, *, gate_act, alpha, seed_t=None, tag=0, thr=0, scale=1.0):
    M, N = g.shape
    out = torch.empty((M, N), device=g.device, dtype=torch.float32)
    check(_lib.lib().mpg_gate(_p(g), g.stride(0), _p(H), 0 if H is None else H.stride(0), _p(out), N, M, N,
                              int(gate_act), alpha, _p(seed_t), tag, thr, scale, _stream()), "mpg_gate")
    return out


def normal_noise_masked(shape, std: float, labels: torch.Tensor, site: int = 0, device="cuda", mean: float = 0.0,
                        mask_out: Optional[torch.Tensor] = None, ignore_out: Optional[torch.Tensor] = None,
                        seed_t: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """``normal_noise`` of a generator's input [B, N, L] AND ``rank_mask`` of its first feature (the jets' masks, mask_c of
    mpgan/model.py:689-699) in one launch: (noise, mask [B, N], 1 - mask [B, N]).  Same values as the two calls.
    ``seed_t`` / ``out``: as ``normal_noise`` takes them."""
    B, N, L = shape
    out = _noise_target(shape, device, out)
    seed_t = _seed_word(seed_t, out.device)
    lab = labels[:, -1]
    if lab.dtype != torch.float32:
        lab = lab.float()
    mask = mask_out if mask_out is not None else torch.empty((B, N), device=device, dtype=torch.float32)
    ign = ignore_out if ignore_out is not None else torch.empty((B, N), device=device, dtype=torch.float32)
    assert mask.is_contiguous() and ign.is_contiguous() and mask.numel() == B * N and ign.numel() == B * N
    check(_lib.lib().mpg_normal_rank_mask(_p(out), B, N, L, _p(seed_t), NOISE_TAG + int(site), mean, std,
                                          _p(lab), lab.stride(0), _p(mask), _p(ign), _stream()), "mpg_normal_rank_mask")
    return out, mask.view(B, N), ign.view(B, N)


# ------------------------------------------------------------------------------------- data feed


def shuffle_indices(key: int, pos0: int, count: int, n: int) -> torch.Tensor:
    """Data-set rows of the stream positions ``pos0 .. pos0 + count - 1`` of the keyed shuffle (``mpg_shuffle_index_host``: the
    kernel's own function compiled for the host, no device involved) as a CPU int64 tensor."""
    out = torch.empty(int(count), dtype=torch.int32)
    check(_lib.lib().mpg_shuffle_index_host(int(key) & 0xFFFFFFFFFFFFFFFF, int(pos0) & 0xFFFFFFFFFFFFFFFF, int(count), int(n),
                                            C.c_void_p(out.data_ptr())), "mpg_shuffle_index_host")
    return out.long()


def batch_feed(particles: torch.Tensor, labels_in: torch.Tensor, key: int, cursor: torch.Tensor, ticket: torch.Tensor, B: int,
               stride: int, data=None, labels=None, dcat=None, x3=None, mask2=None, ign2=None, labels2=None):
    """``mpg_batch_feed``: one launch that gathers the ``B`` jets at the stream positions ``cursor .. cursor + B - 1`` of the keyed
    shuffle from the resident ``particles [n, N, 4]`` / ``labels_in [n]`` into the given buffers (what ``TrainStep.set_batch``
    writes; any may be None) and moves ``cursor`` (one int64 on the device) on by ``stride``."""
    _chk(particles, "particles")
    n, N, F = particles.shape
    if F != 4 or not particles.is_contiguous():
        raise ValueError(f"batch_feed: contiguous particles [n, N, 4] expected, got {tuple(particles.shape)}")
    if cursor.dtype != torch.int64 or ticket.dtype != torch.int32 or cursor.device != particles.device or ticket.device != particles.device:
        raise ValueError("batch_feed: cursor (int64) and ticket (int32) live on the data set's device")
    need = {"data": (data, B * N * 4), "labels": (labels, B), "dcat": (dcat, B * N * 4), "x3": (x3, B * N * 3),
            "mask2": (mask2, B * N), "ign2": (ign2, B * N), "labels2": (labels2, 2 * B), "labels_in": (labels_in, n)}
    for name, (t, k) in need.items():
        if t is not None:
            _chk(t, name)
            if not t.is_contiguous() or t.numel() < k:
                raise ValueError(f"batch_feed: {name} must be contiguous with at least {k} elements, got {tuple(t.shape)}")
    check(_lib.lib().mpg_batch_feed(_p(particles), _p(labels_in), n, N, int(key) & 0xFFFFFFFFFFFFFFFF, C.c_void_p(cursor.data_ptr()),
                                    C.c_void_p(ticket.data_ptr()), int(B), int(stride), _p(data), _p(labels), _p(dcat), _p(x3),
                                    _p(mask2), _p(ign2), _p(labels2), _stream()), "mpg_batch_feed")


# ------------------------------------------------------------------------------------- bulk generation (gen.JetSampler)
CHUNK_SEED_STEP = 0x9E3779B97F4A7C15   # what one chunk adds to a sampler's seed word: seed_c = key + c * CHUNK_SEED_STEP


def chunk_seed(key: int, c: int) -> int:
    """The seed word ``seed_c`` under which chunk ``c`` of a sampler's stream draws its noise (include/mpgan_amd.h)."""
    return (int(key) + int(c) * CHUNK_SEED_STEP) & 0xFFFFFFFFFFFFFFFF


def u64_as_i64(v: int) -> int:
    """The 64-bit pattern ``v`` as the value an int64 tensor holds for it."""
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >= (1 << 63) else v


def label_pick_indices(key: int, pos0: int, count: int, n: int) -> torch.Tensor:
    """Table indices ``idx(g)`` of the stream rows ``pos0 .. pos0 + count - 1`` of a sampler keyed by ``key`` over a table of
    ``n`` labels (``mpg_label_pick_host``: the kernel's own function compiled for the host, no device involved) as a CPU
    int64 tensor."""
    out = torch.empty(max(int(count), 0), dtype=torch.int32)
    check(_lib.lib().mpg_label_pick_host(int(key) & 0xFFFFFFFFFFFFFFFF, int(pos0) & 0xFFFFFFFFFFFFFFFF, int(count), int(n),
                                         C.c_void_p(out.data_ptr()) if out.numel() else None), "mpg_label_pick_host")
    return out.long()


def _stream_words(cursor, ticket, device, what, seed=None):
    if cursor.dtype != torch.int64 or cursor.numel() != 1 or cursor.device != device:
        raise ValueError(f"{what}: cursor is one int64 on {device}")
    if ticket is not None and (ticket.dtype != torch.int32 or ticket.numel() != 1 or ticket.device != device):
        raise ValueError(f"{what}: ticket is one int32 on {device}")
    if seed is not None and (seed.dtype != torch.int64 or seed.numel() != 1 or seed.device != device):
        raise ValueError(f"{what}: seed is one int64 on {device}")


def label_pick(table: torch.Tensor, key: int, cursor: torch.Tensor, B: int, out: torch.Tensor) -> torch.Tensor:
    """``mpg_label_pick``: ``out[b] = table[idx(cursor + b)]`` for the ``B`` jets of a chunk -- labels drawn with replacement
    from the resident 1-D ``table`` by a keyed hash of the stream row (``label_pick_indices`` is its host twin).  ``cursor``
    (one int64 on the device) is read, not moved; ``out``: contiguous, at least ``B`` floats ([B, 1])."""
    _chk(table, "table")
    _chk(out, "out")
    if table.dim() != 1 or not table.is_contiguous() or table.numel() < 1:
        raise ValueError(f"label_pick: a contiguous 1-D table of at least one label expected, got {tuple(table.shape)}")
    if not out.is_contiguous() or out.numel() < int(B) or out.device != table.device:
        raise ValueError(f"label_pick: out must be contiguous with at least {B} elements on {table.device}, got {tuple(out.shape)}")
    _stream_words(cursor, None, table.device, "label_pick")
    check(_lib.lib().mpg_label_pick(_p(table), table.numel(), int(key) & 0xFFFFFFFFFFFFFFFF, C.c_void_p(cursor.data_ptr()), int(B),
                                    _p(out), _stream()), "mpg_label_pick")
    return out


def jets_finish(feat: torch.Tensor, mask: Optional[torch.Tensor], out: torch.Tensor, *, maxes, norms, shifts, key: int,
                cursor: torch.Tensor, seed: torch.Tensor, ticket: torch.Tensor, row0: int = 0, total: Optional[int] = None,
                mask_out: Optional[torch.Tensor] = None, stride: Optional[int] = None) -> torch.Tensor:
    """``mpg_jets_finish``: the un-normalising epilogue of the reference's gen.py:127-141 (``data.unnormalise_jets``, bit for
    bit) on one chunk ``feat [B, N, >= 3]`` (unit feature stride, jets of whole rows: a [B, N, 4] module output is read in place)
    with ``mask [B, N]`` (or None: all real), written into rows ``cursor - row0 ..`` of ``out [total, N, 3]`` (and the 0 / 1
    verdicts into ``mask_out [total, N]``); jets at or beyond ``total`` (default: ``out``'s rows) are not written.  The launch
    then moves ``cursor`` on by B, writes the next chunk's seed word ``chunk_seed(key, cursor / B)`` into ``seed`` and leaves
    ``ticket`` at zero.  ``stride`` (``mpg_jets_finish_stride``; default B): what the cursor moves by instead -- W B for a rank
    of W that share one stream."""
    B, N, F = _jet_layout(feat, "feat")
    _chk(out, "out")
    if feat.stride(0) != N * feat.stride(1) or F < 3:
        raise ValueError(f"jets_finish: feat [B, N, >= 3] with evenly strided particle rows expected (shape {tuple(feat.shape)}, strides {feat.stride()})")
    total = out.shape[0] if total is None else int(total)
    if out.dim() != 3 or out.shape[1:] != (N, 3) or not out.is_contiguous() or not 0 <= total <= out.shape[0] or out.device != feat.device:
        raise ValueError(f"jets_finish: out must be a contiguous [>= {total}, {N}, 3] tensor on {feat.device}, got {tuple(out.shape)}")
    if mask is not None:
        _chk(mask, "mask")
        if not mask.is_contiguous() or mask.numel() != B * N or mask.device != feat.device:
            raise ValueError(f"jets_finish: mask must be contiguous with {B * N} elements, got {tuple(mask.shape)}")
    if mask_out is not None:
        _chk(mask_out, "mask_out")
        if not mask_out.is_contiguous() or mask_out.numel() < total * N or mask_out.device != feat.device:
            raise ValueError(f"jets_finish: mask_out must be contiguous with at least {total * N} elements, got {tuple(mask_out.shape)}")
    _stream_words(cursor, ticket, feat.device, "jets_finish", seed)
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in list(v)[:3]])
    mx, nr, sh = f3(maxes), f3(norms), f3(shifts)
    words = (C.c_void_p(cursor.data_ptr()), C.c_void_p(seed.data_ptr()), C.c_void_p(ticket.data_ptr()), _stream())
    front = (_p(feat), feat.stride(1), _p(mask), B, N, mx, nr, sh, _p(out), _p(mask_out), int(row0) & 0xFFFFFFFFFFFFFFFF, total,
             int(key) & 0xFFFFFFFFFFFFFFFF)
    if stride is None:
        check(_lib.lib().mpg_jets_finish(*front, *words), "mpg_jets_finish")
    else:
        if not 1 <= int(stride) < 2**63:
            raise ValueError(f"jets_finish: stride must be >= 1, got {stride!r}")
        check(_lib.lib().mpg_jets_finish_stride(*front, int(stride), *words), "mpg_jets_finish_stride")
    return out


# ------------------------------------------------------------------------------------- augmentation
AUG_R90, AUG_FLIP, AUG_TRANSLATE, AUG_SCALE = 1, 2, 4, 8   # MPG_AUG_* of include/mpgan_amd.h


def augment_flags(aug_r90=False, aug_f=False, aug_t=False, aug_s=False) -> int:
    """The reference's four switches (``--aug-r90 / -f / -t / -s``) as ``mpg_augment``'s flag bits."""
    return AUG_R90 * bool(aug_r90) + AUG_FLIP * bool(aug_f) + AUG_TRANSLATE * bool(aug_t) + AUG_SCALE * bool(aug_s)


def _jet_layout(x: torch.Tensor, name: str):
    _chk(x, name)
    B, N, F = x.shape
    if x.stride(2) != 1 or x.stride(1) < F or x.stride(0) < N * x.stride(1):
        raise ValueError(f"{name}: rows of unit feature stride, jets of whole rows expected (strides {x.stride()})")
    return B, N, F


def augment_params(B: int, p_tensor: torch.Tensor, flags: int, translate_ratio: float, scale_sd: float, site: int,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The per-jet maps ``augment`` would apply to ``B`` jets at ``site`` under the current seed, [B, 6] =
    (a00, a01, a10, a11, t0, t1), without applying them."""
    _chk(p_tensor, "p_tensor")
    params = out if out is not None else torch.empty((B, 6), device=p_tensor.device, dtype=torch.float32)
    assert params.shape == (B, 6) and params.is_contiguous()
    check(_lib.lib().mpg_augment(None, None, 0, 2, 2, B, 0, _p(seed_tensor(p_tensor.device)), AUG_TAG + int(site), _p(p_tensor),
                                 int(flags), translate_ratio, scale_sd, _p(params), _stream()), "mpg_augment")
    return params


def augment(x: torch.Tensor, p_tensor: torch.Tensor, flags: int, translate_ratio: float, scale_sd: float, site: int,
            out: Optional[torch.Tensor] = None, params: Optional[torch.Tensor] = None):
    """``mpgan.augment.augment`` (train.py:438-442, :508-511) on jets [B, N, F >= 2] as ONE launch: per jet the mixed
    composition of the enabled stages is one affine map of (eta, phi), drawn from the counter-based stream of the device seed
    and ``site`` (0: train_D's generated jets, 1: train_G's, 2: train_D's real jets).  ``p_tensor``: the probability as a
    one-float device tensor.  ``out``: None (a new tensor), ``x`` itself (in place) or a tensor of ``x``'s shape and strides.
    Returns (y, params [B, 6]); no autograd (``AugmentFn``)."""
    B, N, F = _jet_layout(x, "x")
    _chk(p_tensor, "p_tensor")
    if out is None:
        x = x.contiguous()
        out = torch.empty_like(x)
    elif out is not x:
        _jet_layout(out, "out")
        if out.shape != x.shape or out.stride() != x.stride():
            raise ValueError("augment: out must have x's shape and strides")
    if params is None:
        params = torch.empty((B, 6), device=x.device, dtype=torch.float32)
    assert params.shape == (B, 6) and params.is_contiguous()
    check(_lib.lib().mpg_augment(_p(x), _p(out), x.stride(0), x.stride(1), F, B, N, _p(seed_tensor(x.device)), AUG_TAG + int(site),
                                 _p(p_tensor), int(flags), translate_ratio, scale_sd, _p(params), _stream()), "mpg_augment")
    return out, params


# ------------------------------------------------------------------------------------- label smoothing / noise


def label_targets(B: int, smoothing: bool, noise: float, device="cuda", site: int = 0, out=None):
    """``mpg_label_targets``: calc_D_loss's label smoothing / label noise (train.py:341-363) for the 2B jets of a D step under the
    device's current seed, ONE launch.  Returns (targets [2B], extra [1], drawn [2B]): what ``disc_head_loss(targets=,
    loss_extra=)`` and ``train.d_loss(real=, extra=)`` take, and the labels Y as drawn, before the reference's [B, B] broadcast
    (``train.effective_targets`` states the rule).  ``out``: the three tensors to write into."""
    B = int(B)
    if B < 1:
        raise ValueError(f"label_targets: B must be >= 1, got {B}")
    if not 0.0 <= float(noise) <= 1.0:
        raise ValueError(f"label_targets: noise must lie in [0, 1], got {noise!r}")
    if out is None:
        out = (torch.empty(2 * B, device=device, dtype=torch.float32), torch.empty(1, device=device, dtype=torch.float32),
               torch.empty(2 * B, device=device, dtype=torch.float32))
    targets, extra, drawn = out
    for t, k, name in ((targets, 2 * B, "targets"), (extra, 1, "extra"), (drawn, 2 * B, "drawn")):
        _chk(t, name)
        if not t.is_contiguous() or t.numel() != k:
            raise ValueError(f"label_targets: {name} must be contiguous with {k} elements, got {tuple(t.shape)}")
    check(_lib.lib().mpg_label_targets(B, int(bool(smoothing)), float(noise), _p(seed_tensor(targets.device)), LABEL_TAG + int(site),
                                       _p(targets), _p(extra), _p(drawn), _stream()), "mpg_label_targets")
    return targets, extra, drawn


# ------------------------------------------------------------------------------------- adaptive augmentation probability
def ada_update(out: torch.Tensor, n_real: int, mid: float, target: float, step: float, interval: int, state: torch.Tensor,
               aug_p: torch.Tensor, r_out: torch.Tensor):
    """``mpg_ada_update``: ADA's controller of ``augment``'s probability, ONE launch on the current stream.  ``out``: D's per-jet
    outputs of a D step, the real half first (what ``disc_head_loss`` returns; its first ``n_real`` values are read); ``mid``: the
    midpoint of the loss's two targets; ``state``: int32 [2] = (sign sum, D steps counted); ``aug_p`` and ``r_out``: one float32
    each, all three on ``out``'s device.  Adds this step's count of sign(out - mid) to the state and, on the ``interval``-th call,
    moves ``aug_p`` by ``step`` towards 1 (r > ``target``) or 0 (r < ``target``), clamps it to [0, 1], leaves r = sign sum /
    (n_real * interval) in ``r_out`` and clears the state (include/mpgan_amd.h states the rule exactly)."""
    _chk(out, "out")
    n_real, interval = int(n_real), int(interval)
    if not out.is_contiguous() or not 1 <= n_real <= out.numel():
        raise ValueError(f"ada_update: out must be contiguous with at least n_real = {n_real} >= 1 elements, got {tuple(out.shape)}")
    if interval < 1:
        raise ValueError(f"ada_update: interval must be >= 1, got {interval}")
    if n_real * interval > 2**31 - 1:
        raise ValueError(f"ada_update: n_real * interval = {n_real * interval} does not fit the int32 sign sum")
    if not 0.0 <= float(target) <= 1.0:
        raise ValueError(f"ada_update: target must lie in [0, 1], got {target!r}")
    if not float(step) >= 0.0:
        raise ValueError(f"ada_update: step must be >= 0, got {step!r}")
    for t, k, dt, name in ((state, 2, torch.int32, "state"), (aug_p, 1, torch.float32, "aug_p"), (r_out, 1, torch.float32, "r_out")):
        if t.device != out.device or t.dtype != dt or not t.is_contiguous() or t.numel() != k:
            raise ValueError(f"ada_update: {name} must be a contiguous {dt} tensor of {k} element(s) on {out.device}, got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}")
    check(_lib.lib().mpg_ada_update(_p(out), n_real, float(mid), float(target), float(step), interval, _p(state), _p(aug_p), _p(r_out),
                                    _stream()), "mpg_ada_update")


ADA_COUNT_MAX = 1 << 24      # a rank's sign count, and the ranks' sum, stay exact in fp32 up to here


def _ada_words(what: str, device, state, aug_p, r_out):
    for t, k, dt, name in ((state, 2, torch.int32, "state"), (aug_p, 1, torch.float32, "aug_p"), (r_out, 1, torch.float32, "r_out")):
        if t.device != device or t.dtype != dt or not t.is_contiguous() or t.numel() != k:
            raise ValueError(f"{what}: {name} must be a contiguous {dt} tensor of {k} element(s) on {device}, got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}")


def _ada_slot(what: str, device, slot):
    if slot.device != device or slot.dtype != torch.float32 or slot.numel() != 1:
        raise ValueError(f"{what}: slot must be one float32 on {device}, got {slot.dtype} {tuple(slot.shape)} on {slot.device}")


def ada_count(out: torch.Tensor, n_real: int, mid: float, slot: torch.Tensor):
    """``mpg_ada_count``: the first half of ``ada_update`` for data-parallel ranks, ONE launch on the current stream --
    ``slot[0] = float(count of sign(out[:n_real] - mid))``, a store.  ``slot``: one float32 on ``out``'s device (the tail of D's
    flat gradient buffer: the gradient all-reduce adds the ranks' counts)."""
    _chk(out, "out")
    n_real = int(n_real)
    if not out.is_contiguous() or not 1 <= n_real <= out.numel():
        raise ValueError(f"ada_count: out must be contiguous with at least n_real = {n_real} >= 1 elements, got {tuple(out.shape)}")
    if n_real > ADA_COUNT_MAX:
        raise ValueError(f"ada_count: n_real = {n_real} > 2^24: the count would not be exact in the fp32 slot")
    _ada_slot("ada_count", out.device, slot)
    check(_lib.lib().mpg_ada_count(_p(out), n_real, float(mid), _p(slot), _stream()), "mpg_ada_count")


def ada_settle(slot: torch.Tensor, n_real_total: int, target: float, step: float, interval: int, state: torch.Tensor,
               aug_p: torch.Tensor, r_out: torch.Tensor):
    """``mpg_ada_settle``: the second half of ``ada_update``, ONE launch of one thread behind the gradient all-reduce -- the rule
    from ``state[0] += int(slot[0])`` onward with ``n_real_total`` (the real jets of all ranks) in the division.  A slot that is
    not an integer within [-n_real_total, n_real_total] leaves ``state`` and ``aug_p`` untouched and ``r_out`` = NaN."""
    _chk(slot, "slot")
    n_real_total, interval = int(n_real_total), int(interval)
    if n_real_total < 1 or interval < 1:
        raise ValueError(f"ada_settle: n_real_total = {n_real_total} and interval = {interval} must be >= 1")
    if n_real_total * interval > 2**31 - 1:
        raise ValueError(f"ada_settle: n_real_total * interval = {n_real_total * interval} does not fit the int32 sign sum")
    if not 0.0 <= float(target) <= 1.0:
        raise ValueError(f"ada_settle: target must lie in [0, 1], got {target!r}")
    if not float(step) >= 0.0:
        raise ValueError(f"ada_settle: step must be >= 0, got {step!r}")
    _ada_slot("ada_settle", slot.device, slot)
    _ada_words("ada_settle", slot.device, state, aug_p, r_out)
    check(_lib.lib().mpg_ada_settle(_p(slot), n_real_total, float(target), float(step), interval, _p(state), _p(aug_p), _p(r_out),
                                    _stream()), "mpg_ada_settle")


def augment_apply_reference(x: torch.Tensor, params: torch.Tensor) -> torch.Tensor:
    """The torch statement of what ``augment`` applies: y[b, i, :2] = A_b x[b, i, :2] + t_b with
    params[b] = (a00, a01, a10, a11, t0, t1), columns >= 2 unchanged.  Any device and dtype (tests, the CPU path)."""
    a00, a01, a10, a11, t0, t1 = (params[:, k].reshape(-1, 1) for k in range(6))
    x0, x1 = x[..., 0], x[..., 1]
    return torch.cat((torch.stack((a00 * x0 + a01 * x1 + t0, a10 * x0 + a11 * x1 + t1), dim=2), x[..., 2:]), dim=2)


class AugmentFn(torch.autograd.Function):
    """``augment`` with its backward dx = A^T dy (``mpg_augment_bwd``): between a generator's jets and the discriminator in
    train_G.  ``params``: the caller's [B, 6] buffer, which receives the maps.  Returns y."""

    @staticmethod
    def forward(ctx, x, p_tensor, flags, translate_ratio, scale_sd, site, params):
        y, ctx.params = augment(x, p_tensor, flags, translate_ratio, scale_sd, site, params=params)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        B, N, F = dy.shape
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        check(_lib.lib().mpg_augment_bwd(_p(dy), _p(dx), N * F, F, F, B, N, _p(ctx.params), _stream()), "mpg_augment_bwd")
        return dx, None, None, None, None, None, None


def dropout_mask(rows: int, F: int, tag: int, thr: int, device="cuda"):
    """The {0,1} keep mask [rows, F] of dropout site ``tag`` under the current seed (tests)."""
    out = torch.empty((rows, F), device=device, dtype=torch.float32)
    check(_lib.lib().mpg_dropout_mask(_p(out), rows, F, _p(seed_tensor(device)), tag, thr, _stream()),
          "mpg_dropout_mask")
    return out


# ------------------------------------------------------------------------------------- spectral norm
SPECTRAL_MAX = 16    # MPG_SPECTRAL_MAX_JOBS of include/mpgan_amd.h


def _spectral_run(entry, name, jobs, *tail):
    # ``jobs``: filled ``MpgSpectralJob`` / ``MpgSpectralBwdJob`` structs; as many launches as the job limit asks for.
    for i0 in range(0, len(jobs), SPECTRAL_MAX):
        chunk = jobs[i0:i0 + SPECTRAL_MAX]
        check(entry((type(chunk[0]) * len(chunk))(*chunk), len(chunk), *tail), name)


def spectral_norm_launch(layers, power_iterations: int, host: bool = False):
    """``mpg_spectral_norm`` over ``layers`` = [(W_bar [R, C], u [R], v [C]), ...] (``mpg_spectral_norm_host`` on CPU tensors with
    ``host``): power iteration, sigma and W_eff = W_bar / sigma of every layer in ONE launch per ``SPECTRAL_MAX`` layers.  ``u``
    and ``v`` are advanced IN PLACE (``power_iterations`` >= 1).  Returns [(W_eff, u_out, v_out, inv_sigma), ...]: the normalised
    weight and the fresh copies of the vectors and of 1 / sigma that belong to it (include/mpgan_amd.h states the arithmetic)."""
    seen, jobs, outs = set(), [], []
    for W, u, v in layers:
        if W.dim() != 2:
            raise ValueError(f"spectral_norm_launch: W_bar must be a matrix, got {tuple(W.shape)}")
        for t, n, what in ((W, W.numel(), "W_bar"), (u, W.shape[0], "u"), (v, W.shape[1], "v")):
            if t.dtype != torch.float32 or t.is_cuda == host or not t.is_contiguous() or t.numel() != n or t.device != W.device:
                raise ValueError(f"spectral_norm_launch: {what} must be a contiguous float32 tensor of {n} elements on "
                                 f"{'the host' if host else 'the GPU'}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        if u.data_ptr() in seen or v.data_ptr() in seen:
            raise ValueError("spectral_norm_launch: two layers of one call share a power-iteration vector")
        seen.update((u.data_ptr(), v.data_ptr()))
        out = (torch.empty_like(W), torch.empty_like(u), torch.empty_like(v), W.new_empty(1))
        j = _lib.MpgSpectralJob()
        j.W, j.u, j.v, j.R, j.C = _p(W), _p(u), _p(v), W.shape[0], W.shape[1]
        j.W_eff, j.u_out, j.v_out, j.inv_sigma = (_p(t) for t in out)
        jobs.append(j)
        outs.append(out)
    if jobs:
        if host:
            _spectral_run(_lib.lib().mpg_spectral_norm_host, "mpg_spectral_norm_host", jobs, int(power_iterations))
        else:
            _spectral_run(_lib.lib().mpg_spectral_norm, "mpg_spectral_norm", jobs, int(power_iterations), _stream())
    return outs


def spectral_norm_bwd_launch(layers, host: bool = False):
    """``mpg_spectral_norm_bwd`` over ``layers`` = [(G, W_eff, u_out, v_out, inv_sigma, dW, accumulate), ...]:
    dW (+)= (G - <G, W_eff> u v^T) * inv_sigma of every layer in ONE launch per ``SPECTRAL_MAX`` layers."""
    jobs = []
    for G, W_eff, u, v, inv, dW, acc in layers:
        for t in (G, W_eff, u, v, inv, dW):
            if t.dtype != torch.float32 or t.is_cuda == host or not t.is_contiguous():
                raise ValueError("spectral_norm_bwd_launch: contiguous float32 tensors on %s expected" % ("the host" if host else "the GPU"))
        if G.shape != W_eff.shape or dW.shape != W_eff.shape or u.numel() != W_eff.shape[0] or v.numel() != W_eff.shape[1]:
            raise ValueError("spectral_norm_bwd_launch: G, dW [R, C], u [R], v [C] must fit W_eff %s" % (tuple(W_eff.shape),))
        j = _lib.MpgSpectralBwdJob()
        j.G, j.W_eff, j.u, j.v, j.inv_sigma, j.dW = (_p(t) for t in (G, W_eff, u, v, inv, dW))
        j.R, j.C, j.accumulate = W_eff.shape[0], W_eff.shape[1], int(bool(acc))
        jobs.append(j)
    if jobs:
        if host:
            _spectral_run(_lib.lib().mpg_spectral_norm_bwd_host, "mpg_spectral_norm_bwd_host", jobs)
        else:
            _spectral_run(_lib.lib().mpg_spectral_norm_bwd, "mpg_spectral_norm_bwd", jobs, _stream())


class SpectralWeightsFn(torch.autograd.Function):
    """The normalised weights of several spectral-norm layers: ``apply(uv, power_iterations, *W_bars)`` with ``uv`` =
    ((u, v), ...) returns one W_eff per W_bar (``mpg_spectral_norm``, one grouped launch).  The backward (one grouped
    ``mpg_spectral_norm_bwd``) reaches the W_bars only, with the vectors as constants.  It keeps W_eff and the launch's OWN copies
    of u, v and 1 / sigma, never the live vectors: train_D runs two forwards before one backward, and the second forward's power
    iteration writes the parameters' u and v in place."""

    @staticmethod
    def forward(ctx, uv, power_iterations, *Ws):
        outs = spectral_norm_launch([(W.contiguous(), u, v) for W, (u, v) in zip(Ws, uv)], power_iterations)
        ctx.save_for_backward(*(t for out in outs for t in out))
        return tuple(out[0] for out in outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gs):
        saved = ctx.saved_tensors
        grads, jobs = [None] * len(gs), []
        for i, g in enumerate(gs):
            if g is None or not ctx.needs_input_grad[2 + i]:
                continue
            W_eff, u, v, inv = saved[4 * i:4 * i + 4]
            grads[i] = torch.empty_like(W_eff)
            jobs.append((g.contiguous(), W_eff, u, v, inv, grads[i], False))
        spectral_norm_bwd_launch(jobs)
        return (None, None, *grads)


def spectral_weights(layers, power_iterations: int = 1):
    """W_eff = W_bar / sigma of every layer of ``layers`` = [(W_bar, u, v), ...] after ``power_iterations`` steps of the power
    iteration (which advance u and v in place): one launch forwards, one backwards (``SpectralWeightsFn``)."""
    layers = list(layers)
    for W, u, v in layers:
        _chk(W, "W_bar")
    return list(SpectralWeightsFn.apply(tuple((u, v) for _, u, v in layers), int(power_iterations), *(W for W, _, _ in layers)))


# ------------------------------------------------------------------------------------- edge
def pack_weights(W, rows, cols, *, col0=0, transpose=False, scale=1.0, f16=False):
    """bf16 hi/lo fragment image of W[:, col0:col0+cols] (or its transpose)."""
    r, c = (cols, rows) if transpose else (rows, cols)
    MT, QT = (r + 31) // 32, (c + 31) // 32
    img = torch.empty((2 * MT * QT * 2 * 512,), device=W.device, dtype=torch.bfloat16)
    check(_lib.lib().mpg_pack_weights(_p(W, col0), W.stride(0), r, c, int(transpose), scale, int(f16),
                                      C.c_void_p(img.data_ptr()), _stream()), "mpg_pack_weights")
    return img


def _img_elems(rows, cols):
    return 2 * ((rows + 31) // 32) * ((cols + 31) // 32) * 2 * 512   # 16-bit elements of a hi|lo image


PACK_MAX = 24    # MPG_PACK_MAX_JOBS of include/mpgan_amd.h


def refresh_many(packs):
    """Rebuild the weight images of several ``Packed*`` sets (all layers of a network after an optimizer step) with as
    few ``mpg_pack_many`` launches as the job limit allows."""
    todo = [j for pk in packs for j in pk.jobs()]
    for i0 in range(0, len(todo), PACK_MAX):
        chunk = todo[i0:i0 + PACK_MAX]
        jobs = (MpgPackJob * len(chunk))()
        status = C.c_void_p(dev_state(chunk[0][0].device).status.data_ptr())
        for j, (W, rows, cols, tr, scale, f16, rs, sc, img) in zip(jobs, chunk):
            j.W, j.ldw, j.rows, j.cols, j.transpose = _p(W), W.stride(0), rows, cols, tr
            j.scale, j.f16, j.img, j.row_split, j.split_cols = scale, int(f16), C.c_void_p(img.data_ptr()), rs, sc
            j.status = status
        check(_lib.lib().mpg_pack_many(jobs, len(chunk), _stream()), "mpg_pack_many")
    for pk in packs:
        pk._key = pk._current_key()


class _PackedSet:
    """Weight images in persistent buffers, rebuilt by ONE ``mpg_pack_many`` launch.  ``spec``: per image name,
    (W, packed rows, packed cols, transpose, scale, f16, row_split, split_cols); ``params``: the weights the images are made of.

    ``ensure()`` rebuilds when a parameter's storage or autograd version changed (``optimizer.step()``,
    ``load_state_dict``).  Updates made behind torch's back -- ``train.TrainStep`` runs RMSprop on a flat buffer
    through ``mpg_rmsprop`` -- must call ``refresh()`` themselves (TrainStep does, inside its graph segments).
    """

    def __init__(self, params, spec):
        self.params, self._spec = params, spec
        self.img = {k: torch.empty((_img_elems(v[1], v[2]),), device=params[0].device, dtype=torch.bfloat16) for k, v in spec.items()}
        self._key = None

    def _current_key(self):
        return tuple((q.data_ptr(), q._version) for q in self.params)

    def jobs(self):
        """(W, rows, cols, transpose, scale, f16, row_split, split_cols, image) per image."""
        return [v + (self.img[k],) for k, v in self._spec.items()]

    def refresh(self):
        refresh_many([self])

    def ensure(self):
        if self._key != self._current_key():
            self.refresh()
        return self

    def ptr(self, name):
        return C.c_void_p(self.img[name].data_ptr())


class PackedMPLayer(_PackedSet):
    """All weight images one MPLayer call needs (edge network, node network, their transposes and the stacked
    a|c view of fe.net.0)."""

    def __init__(self, params, F, out, dscale, f16, plist=None):
        W1, W2, W3, V1, V2, V3 = params
        self.plist = plist  # the twelve Parameters (W1, b1, ..., V3, c3) when built by MPLayer: .grad targets
        self.F, self.out, self.dscale, self.f16 = F, out, float(dscale), bool(f16)
        KN = V1.shape[1]   # H3 + F (+ the conditioning columns appended to the node network's input)
        super().__init__(params, {
            "W2": (W2, H2, H1, 0, dscale * SC_W2, f16, 0, 0), "W3": (W3, H3, H2, 0, dscale * SC_W3, f16, 0, 0),
            "W3T": (W3, H2, H3, 1, dscale * SC_W3, True, 0, 0), "W2T": (W2, H1, H2, 1, dscale * SC_W2, True, 0, 0),
            "V1": (V1, V1.shape[0], KN, 0, SC_WN, f16, 0, 0), "V2": (V2, V2.shape[0], V2.shape[1], 0, SC_WN, f16, 0, 0),
            "V3": (V3, out, V3.shape[1], 0, SC_WN, f16, 0, 0),
            "V3T": (V3, V3.shape[1], out, 1, 1.0, False, 0, 0), "V2T": (V2, V2.shape[1], V2.shape[0], 1, 1.0, False, 0, 0),
            "V1T": (V1, KN, V1.shape[0], 1, 1.0, False, 0, 0),
            "W1S": (W1, 2 * H1, F, 0, SC_WN, f16, H1, F),        # [a-half ; c-half] of fe.net.0.weight
            "W1ST": (W1, F, 2 * H1, 1, 1.0, False, H1, F),
        })


def chain(M, layers, **kw):
    """mpg_chain front-end.  ``layers``: dicts with img, K, N and optionally bias, nbias, act, drop=(tag,thr,scale),
    gate=(H, act, tag, thr, scale), out (tensor [M, >=N]), wscale (the image holds wscale * W)."""
    run_chain(chain_struct(M, layers, **kw))


def run_chain(c):   # (c: an ``MpgChain`` block, see ``chain_struct``)
    check(_lib.lib().mpg_chain(C.byref(c), _stream()), "mpg_chain")


# = CH_MAXKS * 16 of csrc/chain.hip: the widest layer INPUT (K of any layer, so also N of every layer but the last) a fragment
# buffer of mpg_chain holds -- beyond it the entry point refuses (-2)
CHAIN_MAX_K = 256


def chain_route(c) -> int:
    """Which kernel ``mpg_chain`` would run for the block ``c`` (``_lib.CHAIN_ROUTE_*``), or its negative refusal code;
    host only, nothing is launched."""
    return _lib.lib().mpg_chain_route(C.byref(c))


def chain_struct(M, layers, *, A, lda, K1, A2=None, lda2=0, a_slabs=1, a_slab_stride=0, in_gate=None, in_out=None,
                 alpha=0.2, seed_t=None, f16=False, ascale=1.0):
    """The ``MpgChain`` argument block of ``chain`` (also what ``mpg_edge_fwd_fn`` takes for its epilogue)."""
    c = MpgChain()
    c.A, c.lda, c.K1 = _p(A), lda, K1
    c.A2, c.lda2 = _p(A2), lda2
    c.a_slabs, c.a_slab_stride = a_slabs, a_slab_stride
    if in_gate is not None and in_gate[1]:
        c.in_tag, c.in_thr, c.in_scale = in_gate
    if in_out is not None:
        c.in_out, c.ld_in_out = _p(in_out), in_out.stride(0)
    c.M, c.nlayers, c.alpha, c.seed, c.f16 = M, len(layers), alpha, _p(seed_t), int(f16)
    c.ascale = ascale
    for i, d in enumerate(layers):
        L = c.L[i]
        L.Wimg, L.K, L.N = d["img"], d["K"], d["N"]
        L.wscale = d.get("wscale", 1.0)
        L.bias, L.nbias, L.act = _p(d.get("bias")), d.get("nbias", 0), int(d.get("act", False))
        if d.get("drop") is not None and d["drop"][1]:
            L.drop_tag, L.drop_thr, L.drop_scale = d["drop"]
        if d.get("gate") is not None:
            H, gact, tag, thr, scale = d["gate"]
            L.gateH, L.ldh, L.gate_act = _p(H), H.stride(0), int(gact)
            if thr:
                L.gate_tag, L.gate_thr, L.gate_scale = tag, thr, scale
        if d.get("resid") is not None:
            L.resid, L.ldr = _p(d["resid"]), d["resid"].stride(0)
        if d.get("out") is not None:
            L.out, L.ldo = _p(d["out"]), d["out"].stride(0)
    return c


EDGE_SCALARS = 2          # MPG_EDGE_SCALARS of include/mpgan_amd.h
PARK_BYTES_PER_BLOCK = 10240   # E2 / dZ2 of one (jet, receiver block, sender) block as fp16 fragments: 160 x 32 x 2 bytes
MAX_CHUNK_SENDERS = 160   # mpg_edge_bwd keeps the list of a chunk's unmasked senders in LDS (csrc/edge_bwd.hip)
MAX_CHUNK_SENDERS_ES = 116   # ... with edge scalars (their columns take part of the list's LDS)


def jet_order(mask2d: torch.Tensor) -> torch.Tensor:
    """int32 [B]: the jets by decreasing number of unmasked particles (``mpg_jet_order``).  The last result per device is kept
    and handed out again for a mask with the same storage, shape and version -- the layers of one network pass share their
    mask.  (A stale order would only change in which order workgroups start, never a result: any permutation is valid.)"""
    st = dev_state(mask2d.device)
    key = (mask2d.data_ptr(), tuple(mask2d.shape), mask2d._version)
    hit = getattr(st, "order_cache", None)
    if hit is not None and hit[0] == key:
        return hit[1]
    B, N = mask2d.shape
    order = torch.empty((B,), device=mask2d.device, dtype=torch.int32)
    check(_lib.lib().mpg_jet_order(_p(mask2d), B, N, C.c_void_p(order.data_ptr()), _stream()), "mpg_jet_order")
    st.order_cache = (key, order)
    return order


def _sender_chunks(B, N, max_chunk=None):
    """Sender chunks per (jet, receiver block).  A workgroup costs a 150 KiB LDS fill (about five senders' worth of
    time) plus its chunk's senders, and the 256 CUs take the workgroups of a launch in rounds: the chunk count that
    minimises  rounds * (fill + senders per chunk), with chunks of at least 8 and at most MAX_CHUNK_SENDERS senders
    (B = 256, N = 30: 1 -- every CU already has a workgroup; B = 16, N = 150: 3 -- 240 workgroups in one round, where
    doubling up to 320 workgroups would run two rounds at 62 % occupancy)."""
    RB = (N + 31) // 32
    wg = B * RB
    max_chunk = max_chunk or MAX_CHUNK_SENDERS
    forced = os.environ.get("MPG_FORCE_SC")   # experiments only (load balance of one-round launches)
    if forced:
        return max(int(forced), -(-N // max_chunk))
    best, best_cost = 1, None
    for sc in range(1, max(1, N // 8) + 1):
        per = -(-N // sc)
        if per > max_chunk:
            continue
        cost = -(-wg * sc // 256) * (5 + per)
        if best_cost is None or cost < best_cost:
            best, best_cost = sc, cost
    if best_cost is None:   # (N > 8 * MAX_CHUNK_SENDERS cannot happen below the kernels' own limits; be safe)
        best = -(-N // max_chunk)
    return best


def dw_workgroups(nblk, N):
    """Workgroups of an ``mpg_edge_dw`` launch: one per CU, more when a workgroup would get over 64 blocks.  The blocks are
    dealt in runs of R consecutive senders (csrc/edge_dw.hip), so the bound is R * ceil(nblk / R / nwg) <= 64."""
    R = max(d for d in range(1, 7) if N % d == 0)
    nruns = nblk // R
    return min(nruns, max(256, -(-nruns // (64 // R))))


# What ``FusedMPLayerFn.forward`` saves for its backward, in ``save_for_backward`` order (entries a call has no use for are None) ...
MPLayerSaved = namedtuple("MPLayerSaved", "x2 m1 ac agg h1 h2 W1 b2 b3 W2 W3 V1 V2 V3 sign3 nbr stE2 es wq xf2 order")
# ... and the non-tensor state of the call that the backward needs (``ctx.cfg``)
MPLayerCfg = namedtuple("MPLayerCfg", "B N F agg_scale alpha thr dscale tag SC f16 nq")
# Everything ``FusedMPLayerFn.apply`` takes that is not a tensor with a gradient (see its ``forward``)
MPLayerSettings = namedtuple("MPLayerSettings", "sum_agg alpha p_drop training packed nbr num_knn nq handoff no_grad sparse_ok",
                             defaults=(None, None, 0, 0, None, False, True))
# ... and what a call on the sparse k-NN route saves BEHIND those entries: the rows parked by ``mpg_knn_edge_fwd`` (``knn_saved``)
KnnSaved = namedtuple("KnnSaved", "E1 E2 sign3")


def mplayer_saved(node):
    """The saved tensors of a ``FusedMPLayerFn`` backward node (the ``grad_fn`` behind a fused MPLayer's output), by name."""
    return MPLayerSaved(*node.saved_tensors[:len(MPLayerSaved._fields)])


def knn_saved(node):
    """What a ``FusedMPLayerFn`` backward node of the sparse k-NN route holds beside ``mplayer_saved``: a ``KnnSaved`` (``E1`` [B*N*k, 96]
    and ``E2`` [B*N*k, 160], the inputs of fe.net.1 / fe.net.2 row by row, ``sign3`` [B*N*k, 6, 2] int16); None on the dense routes."""
    tail = node.saved_tensors[len(MPLayerSaved._fields):]
    return KnnSaved(*tail) if tail else None


# The node network's input gradients of one layer -- dz3, dz2, dz1 (at its three pre-activations) and dh0 = [dagg | dx(node path)
# | (conditioning columns)] -- with the ``MpgChain`` block that computes them (None once it has run) ...
FnGrads = namedtuple("FnGrads", "dz3 dz2 dz1 dh0 chain")
# ... and what the backward of the layer ABOVE leaves in ``ctx.pre`` when its data-gradient launch has run that chain already: valid for
# exactly the gradient rows at ``gy_ptr``, which ``keep`` holds alive
FnGradsDone = namedtuple("FnGradsDone", "grads gy_ptr keep")


def _fn_grad_chain(ctx, gy2):
    """Buffers and the ``MpgChain`` block of the node network's input-gradient chain of the layer behind ``ctx`` (the backward
    of mpgan/model.py:279) for the upstream gradient rows ``gy2`` [B*N, out]: an ``FnGrads``."""
    sv, cfg, pk = mplayer_saved(ctx), ctx.cfg, ctx.packed
    V1, V2, V3, alpha, thr, dscale, tag = sv.V1, sv.V2, sv.V3, cfg.alpha, cfg.thr, cfg.dscale, cfg.tag
    V, dev = cfg.B * cfg.N, gy2.device
    n1, n2, out_f = V1.shape[0], V2.shape[0], V3.shape[0]
    dz3 = torch.empty_like(gy2) if thr else gy2
    dz2 = torch.empty((V, n2), device=dev, dtype=torch.float32)
    dz1 = torch.empty((V, n1), device=dev, dtype=torch.float32)
    dh0 = torch.empty((V, V1.shape[1]), device=dev, dtype=torch.float32)  # [dagg | dx(node path) | (conditioning columns)]
    c = chain_struct(V, [dict(img=pk.ptr("V3T"), K=out_f, N=n2, gate=(sv.h2, True, tag + TAG_N1, thr, dscale), out=dz2),
                         dict(img=pk.ptr("V2T"), K=n2, N=n1, gate=(sv.h1, True, tag + TAG_N0, thr, dscale), out=dz1),
                         dict(img=pk.ptr("V1T"), K=n1, N=V1.shape[1], out=dh0)],
                     A=gy2, lda=gy2.stride(0), K1=out_f, in_gate=(tag + TAG_N2, thr, dscale), in_out=dz3 if thr else None,
                     alpha=alpha, seed_t=seed_tensor(dev), f16=False)
    return FnGrads(dz3, dz2, dz1, dh0, c)


def _below_chain(prev, dx, thr, alpha, V):
    """``_fn_grad_chain`` of the layer that produced this layer's input (``prev``: its backward context), fed with this layer's
    ``dx`` rows -- or None when that layer cannot take it: not a fused layer's direct output, another dropout mode or slope,
    another number of rows, no backward pending there."""
    if prev is None or getattr(prev, "cfg", None) is None or getattr(prev, "packed", None) is None:
        return None
    try:
        sv, cfg = mplayer_saved(prev), prev.cfg
    except RuntimeError:   # (already released: its backward has run)
        return None
    if sv.h1 is None or sv.h2 is None or cfg.B * cfg.N != V or sv.V3.shape[0] != dx.shape[1] or (cfg.thr, cfg.alpha) != (thr, alpha):
        return None
    if not any(prev.needs_input_grad):
        return None
    return _fn_grad_chain(prev, dx)


class LayerHandoff:
    """What one fused MPLayer of a network pass receives from the layer below and leaves for the layer above.  The loop over
    the layers (``MPNet._run_layers``) makes one per layer and pass and hands it in as ``handoff=``; nothing is kept on modules
    or tensors.  ``below``: the handoff of the layer below; ``above``: the layer that takes this layer's output; ``next``:
    (PackedMPLayer, fe.net.0.bias) of ``above`` when this layer's launch may project its output rows for it (set by
    ``MPLayer.forward``).  ``FusedMPLayerFn.forward`` leaves ``ac_out`` = (a | c [B*N, 192], the PackedMPLayer whose W1 image
    produced it, data pointer of the rows it was computed from, that set's parameter key) where its edge launch ran that
    projection, and ``node`` = its ``ctx`` (the ``grad_fn`` of its output) when a backward is pending.  Both are offers: the layer
    above takes ``ac_out`` only for those very rows and images, and runs this layer's input-gradient chain in its own backward
    launch (``_below_chain``) only when its ``x`` is that node's output itself -- a hook or a ``.to()`` between two layers costs
    launches, never a value.  A bare ``MPLayer`` called outside such a loop, on another fused layer's output too, gets no handoff
    and so takes one launch per piece, with the same bits."""
    __slots__ = ("below", "above", "next", "ac_out", "node")

    def __init__(self, below=None, above=None):
        self.below, self.above, self.next, self.ac_out, self.node = below, above, None, None, None


# One fused MPLayer call as its helpers see it: the saved tensors by name (an ``MPLayerSaved``; during the forward the one that will be
# saved), the ``MPLayerCfg``, the ``PackedMPLayer`` and the device's seed tensor
MPCall = namedtuple("MPCall", "sv cfg pk seed_t")
# What ``edge_plan`` decides from sizes and switches alone
EdgePlan = namedtuple("EdgePlan", "SC RB need_grad epilogue tickets write_agg lpt")


def edge_plan(B, N, *, es=False, mask=False, need_grad=False, options=None):
    """What one fused MPLayer forward decides from sizes and switches alone (no tensor, no launch), as an ``EdgePlan``: ``SC`` sender
    chunks and ``RB`` receiver blocks per jet; ``epilogue``: the node network is tried as the edge launch's epilogue; ``tickets`` /
    ``write_agg``: that launch needs arrival counters / stores ``agg``; ``lpt``: more workgroups than CUs, handed out heaviest jet
    first (``jet_order``).  ``es`` / ``mask`` / ``need_grad``: the call has edge scalars / a mask / a backward pending; ``options``:
    ``OPTIONS`` as they are now.  Raises when the call would park more than the kernels can address."""
    opt = OPTIONS if options is None else options
    SC = _sender_chunks(B, N, MAX_CHUNK_SENDERS_ES if es else None)
    RB = (N + 31) // 32
    if need_grad and B * RB * N * PARK_BYTES_PER_BLOCK > 0x7fffffff:
        # (mpg_edge_fwd / mpg_edge_bwd return -7: the parked fragments are addressed with 32-bit offsets)
        raise RuntimeError(f"FusedMPLayerFn: {B} jets x {N} particles park {B * RB * N * PARK_BYTES_PER_BLOCK / 2**30:.1f} GiB of "
                           f"edge activations for the backward, beyond the kernels' 2 GiB per launch; split the batch "
                           f"(at most {0x7fffffff // (RB * N * PARK_BYTES_PER_BLOCK)} jets per call at this size)")
    epilogue = bool(opt["fn_epilogue"] and not es and (SC == 1 or opt["fn_chunks"]))
    lpt = bool(mask and opt["lpt_order"] and B * RB * SC > NUM_CUS and B + N + 2 + (B + 63) // 64 * (N + 1) <= 16384)
    # (agg: nobody reads it without a backward, unless the chunks' partial sums travel through its slabs; tickets: the last workgroup
    #  to arrive per (jet, receiver block) adds them up)
    return EdgePlan(SC, RB, bool(need_grad), epilogue, tickets=SC > 1, write_agg=bool(need_grad or SC > 1), lpt=lpt)


def _fill_edge(e, sv, cfg, seed_t):
    # The sixteen fields ``MpgEdgeFwd``, ``MpgEdgeBwd`` and ``MpgEdgeDw`` share, from the call's saved tensors (``sv.ac m1 nbr es wq``),
    # its ``MPLayerCfg`` and the seed tensor.  Returns ``e``.
    e.a, e.c, e.ld_ac, e.mask = _p(sv.ac), _p(sv.ac, H1), 2 * H1, _p(sv.m1)
    e.B, e.N, e.alpha, e.agg_scale = cfg.B, cfg.N, cfg.alpha, cfg.agg_scale
    e.nbr, e.es, e.wq = _p(sv.nbr), _p(sv.es), _p(sv.wq)
    e.seed, e.tag_base, e.thr, e.dscale, e.f16 = _p(seed_t), cfg.tag, cfg.thr, cfg.dscale, int(cfg.f16)
    return e


def _fill_edge_grad(e, sv, dh0, park):
    # The six further fields ``MpgEdgeBwd`` and ``MpgEdgeDw`` share: the upstream gradient of ``agg`` (the head of the ``dh0`` rows), the
    # forward's by-products and the parked dZ2 with its exponents (``park``: an ``EdgeGradBufs``).  Returns ``e``.
    e.dagg, e.ld_dagg = _p(dh0), dh0.stride(0)
    e.sign3, e.stageE2, e.stageZ2, e.gexp = _p(sv.sign3), _p(sv.stE2), _p(park.stZ2), _p(park.gexp)
    return e


# ---- the sparse k-NN route
KNN_MAX_N = 192            # mpg_knn_sets' limit: six neighbour words per receiver
KNN_STAGE_BYTES = 784      # LDS per edge row of mpg_knn_edge_fwd (192 floats + 16 bytes of padding: KNN_STAGE_LD of csrc/knn_edge_impl.h)
KNN_LDS_BYTES = 160 * 1024
KNN_WG_ROWS = int(os.environ.get("MPG_KNN_WG_ROWS", "128"))   # edge rows a workgroup aims for: four tiles of 32, one per wave
KNN_PARK_ROW_BYTES = (H1 + H2) * 4 + 6 * 2 * 2   # E1, E2 in fp32 and the sign words of Z3: what the forward parks per edge row
KNN_GRAD_ROW_BYTES = (H1 + H2 + H3) * 4          # dZ1, dZ2, dZ3 in fp32: what the backward writes per edge row
KnnPlan = namedtuple("KnnPlan", "rows tiles RW workgroups parked_bytes grad_bytes")


def knn_sparse_route(has_nbr, nq, N, k, *, spectral_norm=False, fused=True, double_backward=False, options=None):
    """Does a fused MPLayer call take the sparse k-NN launches?  Only with neighbour sets, the option on, no edge scalars and k < N (k
    = N is the fully connected layer); never a spectral-norm layer, a layer of other widths than [96, 160, 192] with two hidden node
    layers (``fused`` False) or the double-backward route: those stay on the routes they take today.  Host only."""
    opt = OPTIONS if options is None else options
    return bool(has_nbr and opt["knn_sparse"] and nq == 0 and 0 < k < N <= KNN_MAX_N and fused and not spectral_norm and not double_backward)


def knn_block_tiles(N, k, RW):
    """The tiles of one jet under ``RW`` receivers per workgroup: (first edge row, rows) per tile, in workgroup order.  A workgroup's rows
    -- those of its receivers, k each -- are cut into tiles of 32; the last tile of a workgroup may be short."""
    tiles = []
    for i0 in range(0, N, RW):
        r0, nrows = i0 * k, min(RW, N - i0) * k
        tiles += [(r0 + t, min(32, nrows - t)) for t in range(0, nrows, 32)]
    return tiles


def knn_plan(B, N, k, need_grad):
    """What one sparse k-NN MPLayer call decides from sizes alone (no tensor, no launch), as a ``KnnPlan``: ``rows`` = N * k edge rows
    per jet, ``tiles`` of 32 rows per jet, ``RW`` receivers per workgroup, ``workgroups`` of the launch, ``parked_bytes`` the forward
    writes for a backward (0 without one) and ``grad_bytes`` that backward's gradient rows take.  A workgroup takes whole receivers
    -- RW * k rows, about ``KNN_WG_ROWS`` -- and fewer when the launch would otherwise leave CUs idle (2 jets of 150: one receiver
    each).  Raises, before any allocation, when the call would park more than 2 GiB (the dense route's bound) or k is out of range."""
    if not (0 < k <= N <= KNN_MAX_N):
        raise ValueError(f"knn_plan: k = {k} neighbours of N = {N} nodes (0 < k <= N <= {KNN_MAX_N})")
    if B <= 0:
        raise ValueError(f"knn_plan: B = {B}")
    rw_max = max(1, min(N, min(KNN_WG_ROWS, KNN_LDS_BYTES // KNN_STAGE_BYTES) // k))
    fill = [rw for rw in range(1, rw_max + 1) if B * -(-N // rw) >= NUM_CUS]
    RW = max(fill) if fill else min(rw_max, -(-32 // k))   # (too few rows for every CU: at least a tile per workgroup)
    rows = N * k
    parked = B * rows * KNN_PARK_ROW_BYTES if need_grad else 0
    grad = B * rows * KNN_GRAD_ROW_BYTES if need_grad else 0
    if max(parked, grad) > 0x7fffffff:
        raise RuntimeError(f"FusedMPLayerFn (sparse k-NN): {B} jets x {N} particles x {k} neighbours park {max(parked, grad) / 2**30:.1f} GiB "
                           f"of edge rows for the backward, beyond 2 GiB per launch; split the batch "
                           f"(at most {0x7fffffff // (rows * KNN_GRAD_ROW_BYTES)} jets per call at this size)")
    return KnnPlan(rows, len(knn_block_tiles(N, k, RW)), RW, B * -(-N // RW), parked, grad)


def _knn_fwd_desc(call, kp, k, agg, ks):
    # ``MpgKnnEdgeFwd`` of ``call``; ``ks``: the ``KnnSaved`` to park into (entries None: nothing is parked)
    sv, cfg, pk, seed_t = call
    e = MpgKnnEdgeFwd()
    e.a, e.c, e.ld_ac, e.mask, e.nbr = _p(sv.ac), _p(sv.ac, H1), 2 * H1, _p(sv.m1), _p(sv.nbr)
    e.W2img, e.W3img, e.b2, e.b3, e.agg = pk.ptr("W2"), pk.ptr("W3"), _p(sv.b2), _p(sv.b3), _p(agg)
    e.B, e.N, e.k, e.RW, e.alpha, e.agg_scale = cfg.B, cfg.N, k, kp.RW, cfg.alpha, cfg.agg_scale
    e.seed, e.tag_base, e.thr, e.dscale = _p(seed_t), cfg.tag, cfg.thr, cfg.dscale
    e.E1, e.E2, e.sign3 = _p(ks.E1), _p(ks.E2), _p(ks.sign3)
    return e


def _knn_forward(ctx, call, kp, k, biases, y, need_grad):
    # The sparse route's forward launches: ``mpg_knn_edge_fwd`` on the neighbour rows, then the node network (``mpg_chain``) as
    # ``_fwd_two_launches`` runs it.  Returns (agg, the ``KnnSaved``).
    sv, cfg = call.sv, call.cfg
    V, dev = cfg.B * cfg.N, sv.x2.device
    ks = KnnSaved(None, None, None)
    if need_grad:   # (what only a backward reads is not written without one)
        ks = KnnSaved(torch.empty((V * k, H1), device=dev, dtype=torch.float32), torch.empty((V * k, H2), device=dev, dtype=torch.float32),
                      torch.empty((V * k, 6, 2), device=dev, dtype=torch.int16))
    agg = torch.empty((V, H3), device=dev, dtype=torch.float32)
    check(_lib.lib().mpg_knn_edge_fwd(C.byref(_knn_fwd_desc(call, kp, k, agg, ks)), _stream()), "mpg_knn_edge_fwd")
    run_chain(_fn_fwd_chain(call, _fn_fwd_layers(call, biases, y), agg))
    return agg, ks


def _knn_backward(ctx, call, ks, gy2, fng, tg, dx):
    # The sparse route's backward launches: fn's input-gradient chain, ``mpg_knn_edge_bwd`` (the rows' dZ3, dZ2, dZ1, then da | dc in
    # fixed orders), the weight gradients -- fe.net.1 / fe.net.2 from the parked rows as two more jobs of the layer's ONE grouped
    # launch -- and dx through the existing chain.
    sv, cfg, pk, seed_t = call
    kp, k = ctx.knn
    V, dev, need_w = cfg.B * cfg.N, sv.x2.device, tg.W1 is not None
    if fng.chain is not None:
        run_chain(fng.chain)
    dZ1 = torch.empty((V * k, H1), device=dev, dtype=torch.float32)
    dZ2 = torch.empty((V * k, H2), device=dev, dtype=torch.float32) if need_w else None
    dZ3 = torch.empty((V * k, H3), device=dev, dtype=torch.float32) if need_w else None
    dadc = torch.empty((V, 2 * H1), device=dev, dtype=torch.float32)
    e = MpgKnnEdgeBwd()
    e.mask, e.nbr, e.W3Timg, e.W2Timg = _p(sv.m1), _p(sv.nbr), pk.ptr("W3T"), pk.ptr("W2T")
    e.dagg, e.ld_dagg = _p(fng.dh0), fng.dh0.stride(0)
    e.B, e.N, e.k, e.RW, e.alpha, e.agg_scale = cfg.B, cfg.N, k, kp.RW, cfg.alpha, cfg.agg_scale
    e.seed, e.tag_base, e.thr, e.dscale = _p(seed_t), cfg.tag, cfg.thr, cfg.dscale
    e.E1, e.E2, e.sign3 = _p(ks.E1), _p(ks.E2), _p(ks.sign3)
    e.dZ1, e.dZ2, e.dZ3, e.dadc = _p(dZ1), _p(dZ2), _p(dZ3), _p(dadc)
    check(_lib.lib().mpg_knn_edge_bwd(C.byref(e), _stream()), "mpg_knn_edge_bwd")
    sums = SlabSums(dadc[:, :H1], dadc[:, H1:], dadc)
    if need_w:
        acc, wb = tg.direct, WgradBatch()
        wb.add(fng.dz3, sv.h2, out=tg.V3, bias_out=tg.c3, accumulate=acc)
        wb.add(fng.dz2, sv.h1, out=tg.V2, bias_out=tg.c2, accumulate=acc)
        wb.add(fng.dz1, sv.agg, out=tg.V1, out_col0=0, bias_out=tg.c1, accumulate=acc)
        wb.add(fng.dz1, sv.xf2, out=tg.V1, out_col0=H3, accumulate=acc)
        wb.add(sums.da, sv.x2, out=tg.W1, out_col0=0, bias_out=tg.b1, accumulate=acc)
        wb.add(sums.dc, sv.x2, out=tg.W1, out_col0=cfg.F, accumulate=acc)
        wb.add(dZ3, ks.E2, out=tg.W3, bias_out=tg.b3, accumulate=acc)
        wb.add(dZ2, ks.E1, out=tg.W2, bias_out=tg.b2, accumulate=acc)
        st = dev_state(dev)
        side = st.wgrad_stream if acc else None
        if side is not None:   # (as ``_weight_grads``: everything the side stream touches stays referenced until TrainStep joins it)
            st.wgrad_keep.append((sv, ks, gy2, fng[:4], dZ1, dZ2, dZ3, dadc, list(wb.jobs)))
            side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
            wb.flush()
    if dx is not None:
        run_chain(_dx_chain(call, fng.dh0, dx, dadc))


# ---- the edge aggregation as a twice-differentiable op on the row kernels (the gradient penalty, train.py:286-324)
# One MPLayer's  agg_i = s sum_j m_j E3_ij  (DESIGN.md section 4 has the rule):
#   EdgeRowsFn      forward: agg (``mpg_knn_edge_fwd`` over explicit edge rows -- a fully connected layer is k = N with all-ones neighbour
#                   words --, E1 / E2 / sign3 parked); backward: ``EdgeRowsVJPFn.apply``, so the first derivative is itself a node.
#   EdgeRowsVJPFn   forward: x_bar, m_bar and the parameter gradients for a cotangent a_bar (``mpg_knn_edge_bwd``, the dot mode of
#                   ``mpg_knn_edge_jvp``, the weight-gradient GEMMs); backward (once differentiable): the gradients of
#                   Phi = <u, x_bar> + <mu, m_bar> (the jvp mode of ``mpg_knn_edge_jvp``; ``mpg_knn_edge_bwd`` with mu as the mask).
# The gates (dropout keep-and-scale times LeakyReLU') are constants of the call, as they are almost everywhere.  CPU tensors take
# the same formulas in plain torch, in the tensors' dtype, with explicit keep masks: the rule can be checked in fp64 without a GPU.
GP_ROWS_PARK_ROW_BYTES = KNN_PARK_ROW_BYTES + (H1 + H2) * 4 + 2 * KNN_GRAD_ROW_BYTES   # E1 E2 sign3 | T1 T2 | two sets of dZ1..3
# a sender whose mask is exactly 0 is no sender to the row kernels (its rows are neither computed nor parked), but m_bar_j =
# s sum_i <E3_ij, a_bar_i> does not vanish with m_j: where the mask takes a gradient its exact zeros enter the kernels as this factor
ROWS_MASK_FLOOR = 2.0 ** -64
EdgeRowsSettings = namedtuple("EdgeRowsSettings", "sum_agg alpha p_drop training packed nbr k keeps param_grads",
                              defaults=(0.0, True, None, None, 0, None, True))


class PackedEdgeRows(_PackedSet):
    """The weight images ``EdgeRowsFn`` needs, for callers without an MPLayer's ``PackedMPLayer`` (which has them under the same names)."""

    def __init__(self, params, F, dscale, f16):
        W1, W2, W3 = params
        self.F, self.dscale, self.f16 = F, float(dscale), bool(f16)
        super().__init__(params, {
            "W2": (W2, H2, H1, 0, dscale * SC_W2, f16, 0, 0), "W3": (W3, H3, H2, 0, dscale * SC_W3, f16, 0, 0),
            "W3T": (W3, H2, H3, 1, dscale * SC_W3, True, 0, 0), "W2T": (W2, H1, H2, 1, dscale * SC_W2, True, 0, 0),
            "W1S": (W1, 2 * H1, F, 0, SC_WN, f16, H1, F),
        })


def gp_rows_route(B, N, k, *, fused=True, n_es=0, diff_cols=0, spectral_norm=False, batch_norm=False, double_backward=False,
                  options=None):
    """Does an MPLayer call inside ``double_backward_route`` take ``EdgeRowsFn`` instead of the materialised edge matrix?  Only with
    the option on (``OPTIONS["gp_rows"]``), for a layer of the fused widths (``fused``) without edge scalars, difference columns,
    spectral norm or batch norm, N <= ``KNN_MAX_N`` and rows that ``knn_plan`` accepts; ``k`` = N for a fully connected layer.  Host only."""
    opt = OPTIONS if options is None else options
    if not (opt.get("gp_rows") and double_backward and fused and n_es == 0 and not diff_cols and not spectral_norm and not batch_norm):
        return False
    if not (0 < k <= N <= KNN_MAX_N):
        return False
    try:
        knn_plan(B, N, k, True)
    except (ValueError, RuntimeError):
        return False
    return True


class _RowsState:
    """What one ``EdgeRowsFn`` call keeps for its two derivatives beside its saved inputs (constants of the call)."""
    __slots__ = ("cpu", "B", "N", "F", "k", "kp", "nbr", "agg_scale", "alpha", "thr", "dscale", "tag", "pk", "seed_t", "m1",
                 "E1", "E2", "E3", "sign3", "G", "w", "adj", "param_grads")


def _rows_gates_cpu(x, W1, b1, W2, b2, W3, b3, alpha, keeps):
    F = x.shape[-1]
    a, c = x @ W1[:, :F].t() + b1, x @ W1[:, F:2 * F].t()
    one = lambda Z, K: torch.where(Z > 0, torch.ones_like(Z), torch.full_like(Z, alpha)) * (1 if K is None else K)
    K1, K2, K3 = keeps if keeps is not None else (None, None, None)
    Z1 = a.unsqueeze(2) + c.unsqueeze(1)              # [B, i, j, H1]
    G1 = one(Z1, K1); E1 = G1 * Z1
    Z2 = E1 @ W2.t() + b2
    G2 = one(Z2, K2); E2 = G2 * Z2
    Z3 = E2 @ W3.t() + b3
    G3 = one(Z3, K3); E3 = G3 * Z3
    return (G1, G2, G3), (E1, E2, E3)


def _rows_chain_cpu(st, W2, W3, wt, abar):
    # the first-order chain with the per-edge weight ``wt`` [B, i, j, 1] in the mask's place: (dZ1, dZ2, dZ3)
    G1, G2, G3 = st.G
    dZ3 = G3 * (st.agg_scale * wt * abar.unsqueeze(2))
    dZ2 = G2 * (dZ3 @ W3)
    dZ1 = G1 * (dZ2 @ W2)
    return dZ1, dZ2, dZ3


def _outer(dz, e):
    return torch.einsum("bijo,bijk->ok", dz, e)


def _rows_words(B, N, dev):
    return torch.full((B * N, (N + 31) // 32), -1, device=dev, dtype=torch.int32)   # every sender: the fully connected layer


def _rows_bwd_launch(st, mask1, abar2, need_w):
    # ``mpg_knn_edge_bwd`` of the call behind ``st`` with ``mask1`` as the senders' weights: (dZ1, dZ2, dZ3, da | dc)
    V, dev = st.B * st.N, abar2.device
    dZ1 = torch.empty((V * st.k, H1), device=dev, dtype=torch.float32)
    dZ2 = torch.empty((V * st.k, H2), device=dev, dtype=torch.float32) if need_w else None
    dZ3 = torch.empty((V * st.k, H3), device=dev, dtype=torch.float32) if need_w else None
    dadc = torch.empty((V, 2 * H1), device=dev, dtype=torch.float32)
    e = MpgKnnEdgeBwd()
    e.mask, e.nbr, e.W3Timg, e.W2Timg = _p(mask1), _p(st.nbr), st.pk.ptr("W3T"), st.pk.ptr("W2T")
    e.dagg, e.ld_dagg = _p(abar2), abar2.stride(0)
    e.B, e.N, e.k, e.RW, e.alpha, e.agg_scale = st.B, st.N, st.k, st.kp.RW, st.alpha, st.agg_scale
    e.seed, e.tag_base, e.thr, e.dscale = _p(st.seed_t), st.tag, st.thr, st.dscale
    e.E1, e.E2, e.sign3 = _p(st.E1), _p(st.E2), _p(st.sign3)
    e.dZ1, e.dZ2, e.dZ3, e.dadc = _p(dZ1), _p(dZ2), _p(dZ3), _p(dadc)
    check(_lib.lib().mpg_knn_edge_bwd(C.byref(e), _stream()), "mpg_knn_edge_bwd")
    return dZ1, dZ2, dZ3, dadc


def _rows_jvp_desc(st, abar2, b3):
    e = MpgKnnEdgeJvp()
    e.nbr, e.mask, e.dagg, e.ld_dagg = _p(st.nbr), _p(st.m1), _p(abar2), abar2.stride(0)
    e.W2img, e.W3img, e.b3 = st.pk.ptr("W2"), st.pk.ptr("W3"), _p(b3)
    e.E1, e.E2, e.sign3 = _p(st.E1), _p(st.E2), _p(st.sign3)
    e.B, e.N, e.k, e.RW, e.alpha, e.agg_scale = st.B, st.N, st.k, st.kp.RW, st.alpha, st.agg_scale
    e.seed, e.tag_base, e.thr, e.dscale = _p(st.seed_t), st.tag, st.thr, st.dscale
    return e


def _rows_dx(W1, F, dadc):
    # W1a^T da + W1b^T dc  [V, F]
    dx = linear_bwd_data(dadc[:, :H1], W1, w_col0=0, w_cols=F)
    return linear_bwd_data(dadc[:, H1:], W1, w_col0=F, w_cols=F, out=dx, accumulate=True)


class EdgeRowsFn(torch.autograd.Function):
    """agg [B, N, 192] = s sum_j m_j fe([x_i ; x_j]) of one MPLayer (mpgan/model.py:256-267), twice differentiable: see above.
    ``mask``: [B, N] / [B, N, 1] real-valued sender weights or None; ``settings``: an ``EdgeRowsSettings`` -- ``packed`` a
    ``PackedMPLayer`` / ``PackedEdgeRows`` for the call's dropout scale (built for the call when None), ``nbr`` the neighbour words of
    ``knn_sets`` with ``k`` neighbours (None: fully connected); on the CPU ``nbr`` is a 0/1 adjacency [B, N, N] and ``keeps`` the three
    keep-and-scale masks [B, N, N, 96 / 160 / 192] (None: no dropout).  ``param_grads`` False: a first derivative taken with
    ``create_graph=True`` leaves the parameter gradients out (None) -- the penalty differentiates with respect to the input alone
    there (train.py:304-311), and four GEMMs over all edge rows would be formed for nobody; a plain backward through the op (the
    penalty's own backward reaches it again: D's pooled output and the next layer's input depend on agg) always has them."""

    @staticmethod
    def forward(ctx, x, mask, W1, b1, W2, b2, W3, b3, settings):
        s = settings
        B, N, F = x.shape
        st = _RowsState()
        st.cpu, st.B, st.N, st.F, st.alpha, st.param_grads = not x.is_cuda, B, N, F, float(s.alpha), bool(s.param_grads)
        st.k = int(s.k) if s.nbr is not None else N
        st.agg_scale = 1.0 if s.sum_agg else 1.0 / st.k
        ctx.st, ctx.mask_shape = st, None if mask is None else tuple(mask.shape)
        ctx.save_for_backward(x, mask, W1, b1, W2, b2, W3, b3)
        if st.cpu:
            st.G, E = _rows_gates_cpu(x, W1, b1, W2, b2, W3, b3, st.alpha, s.keeps)
            st.E1, st.E2, st.E3 = E
            st.adj = torch.ones((B, N, N, 1), dtype=x.dtype) if s.nbr is None else s.nbr.to(x.dtype).reshape(B, N, N, 1)
            st.w = st.adj if mask is None else st.adj * mask.reshape(B, 1, N, 1)
            return st.agg_scale * (st.w * st.E3).sum(2)
        _chk(x, "x")
        V, dev = B * N, x.device
        st.kp = knn_plan(B, N, st.k, True)   # (raises before any allocation or launch)
        st.thr, st.dscale = drop_params(s.p_drop) if s.training else (0, 1.0)
        st.seed_t, st.tag = seed_tensor(dev), next_tag(dev, "edge_rows", st.thr)
        pk = s.packed
        if pk is None or pk.dscale != st.dscale or pk.f16 != FWD_F16:
            pk = PackedEdgeRows((W1, W2, W3), F, st.dscale, FWD_F16)
        st.pk = pk.ensure()
        st.nbr = s.nbr if s.nbr is not None else _rows_words(B, N, dev)
        x2 = _unit_cols(x.reshape(V, F))
        st.m1 = None
        if mask is not None:
            st.m1 = mask.detach().reshape(V).contiguous()
            if ctx.needs_input_grad[1]:
                st.m1 = torch.where(st.m1 == 0, torch.full_like(st.m1, ROWS_MASK_FLOOR), st.m1)
        ac = torch.empty((V, 2 * H1), device=dev, dtype=torch.float32)
        run_chain(_ac_chain(st.pk, b1, x2, ac, MPLayerCfg(B, N, F, st.agg_scale, st.alpha, st.thr, st.dscale, st.tag, 1, FWD_F16, 0)))
        st.E1 = torch.empty((V * st.k, H1), device=dev, dtype=torch.float32)
        st.E2 = torch.empty((V * st.k, H2), device=dev, dtype=torch.float32)
        st.sign3 = torch.empty((V * st.k, 6, 2), device=dev, dtype=torch.int16)
        agg = torch.empty((V, H3), device=dev, dtype=torch.float32)
        e = MpgKnnEdgeFwd()
        e.a, e.c, e.ld_ac, e.mask, e.nbr = _p(ac), _p(ac, H1), 2 * H1, _p(st.m1), _p(st.nbr)
        e.W2img, e.W3img, e.b2, e.b3, e.agg = st.pk.ptr("W2"), st.pk.ptr("W3"), _p(b2), _p(b3), _p(agg)
        e.B, e.N, e.k, e.RW, e.alpha, e.agg_scale = B, N, st.k, st.kp.RW, st.alpha, st.agg_scale
        e.seed, e.tag_base, e.thr, e.dscale = _p(st.seed_t), st.tag, st.thr, st.dscale
        e.E1, e.E2, e.sign3 = _p(st.E1), _p(st.E2), _p(st.sign3)
        check(_lib.lib().mpg_knn_edge_fwd(C.byref(e), _stream()), "mpg_knn_edge_fwd")
        return agg.reshape(B, N, H3)

    @staticmethod
    def backward(ctx, abar):
        x, mask, W1, b1, W2, b2, W3, b3 = ctx.saved_tensors
        need = ctx.needs_input_grad
        again = torch.is_grad_enabled()     # (create_graph=True: this derivative will be differentiated itself)
        flags = (need[0], mask is not None and need[1], any(need[2:8]) and (ctx.st.param_grads or not again), again)
        out = EdgeRowsVJPFn.apply(abar, x, mask, W1, b1, W2, b2, W3, b3, ctx.st, flags, ctx.mask_shape)
        return (*out, None)


class EdgeRowsVJPFn(torch.autograd.Function):
    """The first derivative of ``EdgeRowsFn`` as a function of (a_bar, x, mask, parameters): (x_bar, m_bar, W1_bar, b1_bar, ...,
    b3_bar).  Its own backward takes cotangents ``u`` on x_bar and ``mu`` on m_bar -- one on a parameter gradient raises -- and is
    once differentiable: a third derivative declines loudly."""

    @staticmethod
    def forward(ctx, abar, x, mask, W1, b1, W2, b2, W3, b3, st, flags, mask_shape):
        need_x, need_m, need_w, again = flags
        ctx.st, ctx.flags, ctx.mask_shape = st, flags, mask_shape
        ctx.set_materialize_grads(False)
        B, N, F = st.B, st.N, st.F
        if st.cpu:
            ctx.save_for_backward(abar, x, mask, W1, W2, W3)
            dZ1, dZ2, dZ3 = _rows_chain_cpu(st, W2, W3, st.w, abar)
            da, dc = dZ1.sum(2), dZ1.sum(1)
            xbar = da @ W1[:, :F] + dc @ W1[:, F:2 * F]
            mbar = None
            if need_m:
                mbar = (st.agg_scale * (st.adj * st.E3 * abar.unsqueeze(2)).sum((1, 3))).reshape(mask_shape)
            pg = (None,) * 6
            if need_w:
                pg = (torch.cat((da.reshape(-1, H1).t() @ x.reshape(-1, F), dc.reshape(-1, H1).t() @ x.reshape(-1, F)), 1),
                      da.sum((0, 1)), _outer(dZ2, st.E1), dZ2.sum((0, 1, 2)), _outer(dZ3, st.E2), dZ3.sum((0, 1, 2)))
            ctx.dz = (dZ1, dZ2, dZ3)
            return (xbar, mbar, *pg)
        V = B * N
        abar2 = abar.reshape(V, H3).contiguous()
        x2 = _unit_cols(x.reshape(V, F))
        dZ1, dZ2, dZ3, dadc = _rows_bwd_launch(st, st.m1, abar2, need_w or again)
        ctx.save_for_backward(abar2, x2, W1, b3)
        ctx.dz = (dZ1, dZ2, dZ3, dadc) if again else None
        xbar = _rows_dx(W1, F, dadc).reshape(B, N, F) if need_x else None
        mbar = None
        if need_m:
            rowdot = torch.empty((V * st.k,), device=x.device, dtype=torch.float32)
            mbar = torch.empty((V,), device=x.device, dtype=torch.float32)
            e = _rows_jvp_desc(st, abar2, b3)
            e.rowdot, e.dmask = _p(rowdot), _p(mbar)
            check(_lib.lib().mpg_knn_edge_jvp(C.byref(e), _stream()), "mpg_knn_edge_jvp")
            mbar = mbar.reshape(mask_shape)
        pg = (None,) * 6
        if need_w:
            dev = x.device
            g1 = torch.empty_like(W1); gb1 = torch.empty_like(b1)
            g2 = torch.empty_like(W2); gb2 = torch.empty_like(b2)
            g3 = torch.empty_like(W3); gb3 = torch.empty_like(b3)
            wb = WgradBatch()
            wb.add(dadc[:, :H1], x2, out=g1, out_col0=0, bias_out=gb1)
            wb.add(dadc[:, H1:], x2, out=g1, out_col0=F)
            wb.add(dZ2, st.E1, out=g2, bias_out=gb2)
            wb.add(dZ3, st.E2, out=g3, bias_out=gb3)
            wb.flush()
            pg = (g1, gb1, g2, gb2, g3, gb3)
        return (xbar, mbar, *pg)

    @staticmethod
    @once_differentiable
    def backward(ctx, u, mu, *gparams):
        if any(g is not None for g in gparams):
            raise RuntimeError("EdgeRowsVJPFn: a cotangent arrived on a parameter-gradient output; the second-order rule covers the "
                               "input gradient and the mask gradient only")
        st = ctx.st
        B, N, F = st.B, st.N, st.F
        _, n_x, n_m, n_W1, n_b1, n_W2, n_b2, n_W3, n_b3 = ctx.needs_input_grad[:9]
        if st.cpu:
            abar, x, mask, W1, W2, W3 = ctx.saved_tensors
            dZ1, dZ2, dZ3 = ctx.dz
            G1, G2, G3 = st.G
            if u is None:
                u = torch.zeros_like(x)
            P = (u @ W1[:, :F].t()).unsqueeze(2) + (u @ W1[:, F:2 * F].t()).unsqueeze(1)
            T1 = G1 * P
            T2 = G2 * (T1 @ W2.t())
            T3 = G3 * (T2 @ W3.t())
            g_abar = st.w * T3
            g_m = None
            if mask is not None:
                g_m = (st.agg_scale * (st.adj * T3 * abar.unsqueeze(2)).sum((1, 3))).reshape(ctx.mask_shape)
            da, dc = dZ1.sum(2).reshape(-1, H1), dZ1.sum(1).reshape(-1, H1)
            u2, x2 = u.reshape(-1, F), x.reshape(-1, F)
            g_W1 = torch.cat((da.t() @ u2, dc.t() @ u2), 1)
            g_W2, g_W3 = _outer(dZ2, T1), _outer(dZ3, T2)
            g_x = g_b1 = g_b2 = g_b3 = None
            if mu is not None:
                wmu = st.adj * mu.reshape(B, 1, N, 1)
                g_abar = g_abar + wmu * st.E3
                tZ1, tZ2, tZ3 = _rows_chain_cpu(st, W2, W3, wmu, abar)
                ta, tc = tZ1.sum(2), tZ1.sum(1)
                g_x = ta @ W1[:, :F] + tc @ W1[:, F:2 * F]
                g_W1 = g_W1 + torch.cat((ta.reshape(-1, H1).t() @ x2, tc.reshape(-1, H1).t() @ x2), 1)
                g_W2, g_W3 = g_W2 + _outer(tZ2, st.E1), g_W3 + _outer(tZ3, st.E2)
                g_b1, g_b2, g_b3 = ta.sum((0, 1)), tZ2.sum((0, 1, 2)), tZ3.sum((0, 1, 2))
            g_abar = st.agg_scale * g_abar.sum(2)
            return (g_abar, g_x, g_m, g_W1, g_b1, g_W2, g_b2, g_W3, g_b3, None, None, None)
        abar2, x2, W1, b3 = ctx.saved_tensors
        if ctx.dz is None:
            raise RuntimeError("EdgeRowsVJPFn: the first derivative was taken without create_graph=True; there is nothing to differentiate again")
        dZ1, dZ2, dZ3, dadc = ctx.dz
        V, dev = B * N, abar2.device
        need_w = n_W1 or n_W2 or n_W3 or n_b1 or n_b2 or n_b3
        u2 = torch.zeros((V, F), device=dev, dtype=torch.float32) if u is None else _unit_cols(u.reshape(V, F).float())
        # the tangent projections, without bias; bf16 hi + lo operands: a cotangent has no fixed magnitude
        ta = linear_fwd(u2, W1, None, w_col0=0, w_cols=F, f16=False)
        tc = linear_fwd(u2, W1, None, w_col0=F, w_cols=F, f16=False)
        rows = V * st.k
        T1 = torch.empty((rows, H1), device=dev, dtype=torch.float32) if need_w else None
        T2 = torch.empty((rows, H2), device=dev, dtype=torch.float32) if need_w else None
        g_abar = torch.empty((V, H3), device=dev, dtype=torch.float32)
        want_m = st.m1 is not None and n_m
        rowdot = torch.empty((rows,), device=dev, dtype=torch.float32) if want_m else None
        g_m = torch.empty((V,), device=dev, dtype=torch.float32) if want_m else None
        mu1 = None if mu is None else mu.reshape(V).contiguous().float()
        e = _rows_jvp_desc(st, abar2, b3)
        e.mu, e.ta, e.tc, e.ld_t = _p(mu1), _p(ta), _p(tc), ta.stride(0)
        e.T1, e.T2, e.aggt, e.rowdot, e.dmask = _p(T1), _p(T2), _p(g_abar), _p(rowdot), _p(g_m)
        check(_lib.lib().mpg_knn_edge_jvp(C.byref(e), _stream()), "mpg_knn_edge_jvp")
        g_x = tdz = None
        if mu1 is not None:   # the first-order chain once more, mu in the mask's place (it may be negative: the kernel tests != 0)
            tdz = _rows_bwd_launch(st, mu1, abar2, need_w)
            if n_x:
                g_x = _rows_dx(W1, F, tdz[3]).reshape(B, N, F)
        pg = (None,) * 6
        if need_w:
            W2s, W3s = st.pk.params[1], st.pk.params[2]
            g1 = torch.empty_like(W1); g2 = torch.empty_like(W2s); g3 = torch.empty_like(W3s)
            gb = [None, None, None]
            wb = WgradBatch()
            wb.add(dadc[:, :H1], u2, out=g1, out_col0=0)
            wb.add(dadc[:, H1:], u2, out=g1, out_col0=F)
            wb.add(dZ2, T1, out=g2)
            wb.add(dZ3, T2, out=g3)
            if tdz is not None:
                tZ1, tZ2, tZ3, tdadc = tdz
                gb = [torch.zeros((h,), device=dev, dtype=torch.float32) for h in (H1, H2, H3)]   # (their jobs add: the tangent stream has no bias)
                wb.add(tdadc[:, :H1], x2, out=g1, out_col0=0, bias_out=gb[0], accumulate=True)
                wb.add(tdadc[:, H1:], x2, out=g1, out_col0=F, accumulate=True)
                wb.add(tZ2, st.E1, out=g2, bias_out=gb[1], accumulate=True)
                wb.add(tZ3, st.E2, out=g3, bias_out=gb[2], accumulate=True)
            wb.flush()
            pg = (g1, gb[0], g2, gb[1], g3, gb[2])
        g_m = None if g_m is None else g_m.reshape(ctx.mask_shape)
        return (g_abar.reshape(B, N, H3), g_x, g_m, *pg, None, None, None)


# ---- forward
def _unit_cols(t):
    return t if t.stride(1) == 1 else t.contiguous()   # (every consumer takes the row stride, only unit column stride matters)


def _row_views(x, mask, xfn):
    # (x2 [V, F], m1 [V] or None, xf2 [V, F + E]): the nodes, their mask and the node network's view of the nodes as rows.
    V = x.shape[0] * x.shape[1]
    x2 = _unit_cols(x.reshape(V, -1))   # a view when x is a feature slice of a contiguous tensor (D's x[..., :-1])
    m1 = None if mask is None else mask.reshape(V).contiguous()
    return x2, m1, x2 if xfn is None else _unit_cols(xfn.detach().reshape(V, -1))


def _edge_scalar_terms(es, W1, cfg):
    # (es [B, N, EDGE_SCALARS, N] contiguous, wq [EDGE_SCALARS, H1] = their columns of fe.net.0.weight), or (None, None).
    if es is None:
        return None, None
    B, N, F, nq = cfg.B, cfg.N, cfg.F, cfg.nq
    assert 0 < nq <= EDGE_SCALARS and tuple(es.shape) == (B, N, EDGE_SCALARS, N) and W1.shape[1] == 2 * F + nq
    wq = torch.zeros((EDGE_SCALARS, H1), device=W1.device, dtype=torch.float32)
    wq[:nq] = W1.detach()[:, 2 * F:2 * F + nq].t()
    return es.detach().float().contiguous(), wq


def _ac_chain(pk, b1, rows, ac, cfg):
    # The ``MpgChain`` of a layer's node terms ``ac`` = a | c = rows [W1a ; W1c]^T (+ b1 on the a half); ``pk``: that layer's images.
    F = rows.shape[1]
    return chain_struct(rows.shape[0], [dict(img=pk.ptr("W1S"), K=F, N=2 * H1, bias=b1, nbias=H1, out=ac, wscale=SC_WN)],
                        A=rows, lda=rows.stride(0), K1=F, alpha=cfg.alpha, f16=cfg.f16, ascale=SC_ACT)


def _node_terms(below, pk, x2, b1, cfg):
    # Layer-1 node terms a | c [V, 2 * H1] of the rows ``x2``: handed over by the launch that produced x (``below.ac_out``, valid for
    # these very rows and the weight images as they are now), or one launch.
    shape = (x2.shape[0], 2 * H1)
    if below is not None and below.ac_out is not None:
        ac, pk_pre, x_ptr, key_pre = below.ac_out
        if pk_pre is pk and key_pre == pk._key and x_ptr == x2.data_ptr() and tuple(ac.shape) == shape:
            return ac
    ac = torch.empty(shape, device=x2.device, dtype=torch.float32)
    run_chain(_ac_chain(pk, b1, x2, ac, cfg))
    return ac


def _edge_fwd_desc(call, aggp):
    # ``MpgEdgeFwd`` of ``call`` with ``agg`` = ``aggp`` [SC, V, H3], or None for a launch that stores none.
    sv, cfg, pk, seed_t = call
    e = _fill_edge(MpgEdgeFwd(), sv, cfg, seed_t)
    e.W2img, e.W3img, e.b2, e.b3 = pk.ptr("W2"), pk.ptr("W3"), _p(sv.b2), _p(sv.b3)
    e.agg, e.SC, e.skip_masked = _p(aggp), cfg.SC, int(OPTIONS["skip_masked"])
    # E2 (the second edge layer's output) parked as fp16 fragments for the backward, which takes LeakyReLU' from its signs
    # instead of recomputing the layer, and for the weight-gradient kernel
    e.sign3, e.stageE2, e.order = _p(sv.sign3), _p(sv.stE2), _p(sv.order)
    # product form of the edge layers (MpgEdgeFwd.two_term; edge scalars ride on the three-term kernels only)
    e.two_term = int(OPTIONS["fwd_two_term"]) if sv.es is None else 0
    return e


def _fn_fwd_layers(call, biases, y):
    # The node network fn (mpgan/model.py:279) as three chained layers that end in ``y``; h1 / h2 are stored only for a backward.
    sv, cfg, pk, _ = call
    (n1, k1), n2, n3, tag, drop = sv.V1.shape, sv.V2.shape[0], sv.V3.shape[0], cfg.tag, (cfg.thr, cfg.dscale)
    return [dict(img=pk.ptr("V1"), K=k1, N=n1, bias=biases[0], act=True, drop=(tag + TAG_N0, *drop), out=sv.h1, wscale=SC_WN),
            dict(img=pk.ptr("V2"), K=n1, N=n2, bias=biases[1], act=True, drop=(tag + TAG_N1, *drop), out=sv.h2, wscale=SC_WN),
            dict(img=pk.ptr("V3"), K=n2, N=n3, bias=biases[2], act=False, drop=(tag + TAG_N2, *drop), out=y, wscale=SC_WN)]


def _fn_fwd_chain(call, fn_layers, agg):
    # ``MpgChain`` of the node network on [agg | xf2] rows.
    sv, cfg, _, seed_t = call
    return chain_struct(cfg.B * cfg.N, fn_layers, A=agg, lda=H3, K1=H3, A2=sv.xf2, lda2=sv.xf2.stride(0), alpha=cfg.alpha,
                        seed_t=seed_t, f16=cfg.f16, ascale=SC_ACT)


def _next_node_terms(handoff, y, cfg):
    # (ac_next, the next layer's PackedMPLayer, the ``MpgChain`` of its a | c projection of the rows ``y``) where the epilogue form may
    # append that projection, else None.
    out_f = y.shape[1]
    pk_n, b1_n = handoff.next if handoff is not None and handoff.next is not None else (None, None)
    if pk_n is None or out_f % 4 or out_f > 32 or pk_n.F != out_f or pk_n.f16 != cfg.f16:
        return None
    pk_n.ensure()
    ac_next = torch.empty((y.shape[0], 2 * H1), device=y.device, dtype=torch.float32)
    return ac_next, pk_n, _ac_chain(pk_n, b1_n, y, ac_next, cfg)


_NOT_COVERED = object()   # what a route returns when its kernel answers MPG_FN_NA: not one of its shapes


def _fwd_epilogue(call, plan, aggp, fn_layers, handoff):
    # The edge network with the node network -- and the next layer's a | c projection -- as the epilogue of ONE launch
    # (``mpg_edge_fwd_fn``: a whole jet per workgroup or ticketed sender chunks, the default widths).  Returns ``agg`` (None when no
    # backward will read it), or ``_NOT_COVERED``.
    e = _edge_fwd_desc(call, aggp if plan.write_agg else None)
    if plan.tickets:
        e.tickets = _p(_tickets(aggp.device, call.cfg.B * plan.RB))   # arrival counters of the (jet, receiver block)s: zero, and left zero
    cs = _fn_fwd_chain(call, fn_layers, aggp)
    y = fn_layers[-1]["out"]
    nxt = _next_node_terms(handoff, y, call.cfg)
    rc = _lib.lib().mpg_edge_fwd_fn(C.byref(e), C.byref(cs), None if nxt is None else C.byref(nxt[2]), _stream())
    if rc == _lib.MPG_FN_NA:
        return _NOT_COVERED
    check(rc, "mpg_edge_fwd_fn")
    if nxt is not None:
        handoff.ac_out = (nxt[0], nxt[1], y.data_ptr(), nxt[1]._key)
    return aggp[0] if plan.need_grad else None   # (SC > 1: the last workgroup to arrive left the chunks' total in slab 0)


def _fwd_two_launches(call, aggp, fn_layers):
    # ``mpg_edge_fwd``, the chunks' sum, ``mpg_chain`` (fn): every shape.  Returns ``agg``.
    check(_lib.lib().mpg_edge_fwd(C.byref(_edge_fwd_desc(call, aggp)), _stream()), "mpg_edge_fwd")
    agg = aggp[0]
    for q in range(1, call.cfg.SC):   # (in chunk order, slab by slab: the order the epilogue form's last arriver takes -- the two routes
        agg = agg + aggp[q]           #  then agree bit for bit; torch.sum over the chunk axis adds in another order)
    run_chain(_fn_fwd_chain(call, fn_layers, agg))
    return agg


def _leave_offers(ctx, handoff, x, need_grad):
    # What the backwards of this layer and of its neighbours find: ``ctx.prev_node`` (x is the very output of the layer below: this
    # layer's backward may run that layer's input-gradient chain in its own launch), ``ctx.pre`` (filled by the backward of the
    # layer ABOVE when it has run this layer's input-gradient chain already) and ``handoff.node``.
    below = handoff.below if handoff is not None else None
    ctx.prev_node = below.node if (below is not None and need_grad and x.grad_fn is below.node) else None
    ctx.pre = None
    if handoff is not None and need_grad:
        handoff.node = ctx


# ---- backward
# The twelve parameter-gradient targets of one backward: the parameters' .grad buffers (``direct``: added into, and autograd gets
# None) or fresh tensors; all None when no parameter wants a gradient
MPGradTargets = namedtuple("MPGradTargets", "W1 b1 W2 b2 W3 b3 V1 c1 V2 c2 V3 c3 direct")
# Buffers of the edge network's backward: the chunks' partial da [SC, V, H1] and the receiver blocks' partial dc [RB, V, H1]; dZ2 parked
# as fp16 fragments (as the lanes hold them) with the gradient-unit exponent per (jet, receiver block), for a weight-gradient pass
# only; the edge scalars' gradient and their columns' partials
EdgeGradBufs = namedtuple("EdgeGradBufs", "dap dcp stZ2 gexp des daq")
SlabSums = namedtuple("SlabSums", "da dc dadc")   # da, dc [V, H1]; dadc [V, 2 * H1] where they were summed into one buffer, else None


def _taken_fn_grads(ctx, gy2):
    # The ``FnGrads`` the layer above has left in ``ctx.pre`` -- if it ran the chain for exactly this upstream gradient -- else None.
    pre, ctx.pre = ctx.pre, None
    ok = pre is not None and pre.gy_ptr == gy2.data_ptr() and gy2.shape == pre.grads.dz3.shape   # (dz3 [V, out]: rows as its upstream's)
    return pre.grads._replace(chain=None) if ok else None


def _grad_targets(call, need_w):
    # DeviceState.grad_into_param: add into the parameters' .grad buffers directly (the layer must know its twelve Parameters:
    # ``pk.plist``) and return None for them.  Returns (the MPGradTargets, the ParamGrads whose slots autograd gets).
    sv, pk = call.sv, call.pk
    pg = ParamGrads(dev_state(sv.x2.device), pk.plist or (None,) * 12, (need_w,) * 12, eligible=pk.plist is not None)
    tg, direct = pg.written(lambda: [t for W in (sv.W1, sv.W2, sv.W3, sv.V1, sv.V2, sv.V3) for t in (torch.empty_like(W), W.new_empty(W.shape[0]))])
    return MPGradTargets(*tg, direct=bool(direct)), pg


def _edge_grad_bufs(call, need_w):
    sv, cfg = call.sv, call.cfg
    V, RB, dev = cfg.B * cfg.N, (cfg.N + 31) // 32, sv.x2.device
    stZ2 = torch.empty((cfg.B * RB * cfg.N, H2, 32), device=dev, dtype=torch.float16) if need_w else None
    gexp = torch.empty((cfg.B * RB,), device=dev, dtype=torch.int32) if need_w else None
    des = None if sv.es is None else torch.zeros_like(sv.es)   # (zero-masked senders' rows are not written)
    daq = None if sv.es is None else torch.empty((cfg.SC, V, EDGE_SCALARS, H1), device=dev, dtype=torch.float32)
    return EdgeGradBufs(torch.empty((cfg.SC, V, H1), device=dev, dtype=torch.float32),
                        torch.empty((RB, V, H1), device=dev, dtype=torch.float32), stZ2, gexp, des, daq)


def _edge_bwd_desc(call, dh0, bufs):
    sv, cfg, pk, seed_t = call
    e = _fill_edge_grad(_fill_edge(MpgEdgeBwd(), sv, cfg, seed_t), sv, dh0, bufs)
    e.W2img, e.W3Timg, e.W2Timg, e.b2 = pk.ptr("W2"), pk.ptr("W3T"), pk.ptr("W2T"), _p(sv.b2)
    e.SC, e.order, e.des, e.daq = cfg.SC, _p(sv.order), _p(bufs.des), _p(bufs.daq)
    e.da, e.dc = _p(bufs.dap), _p(bufs.dcp)
    return e


def _edge_dw_desc(call, dh0, bufs, tg, part):
    # ``MpgEdgeDw``: the gradients of fe.net.1 / fe.net.2 into ``tg``, through the per-workgroup partials ``part`` [nwg, ...].
    sv, cfg, _, seed_t = call
    d = _fill_edge_grad(_fill_edge(MpgEdgeDw(), sv, cfg, seed_t), sv, dh0, bufs)
    d.part, d.nwg = _p(part), part.shape[0]
    d.dW3, d.dW2, d.db3, d.db2, d.accumulate = _p(tg.W3), _p(tg.W2), _p(tg.b3), _p(tg.b2), int(tg.direct)
    d.defer_reduce = int(OPTIONS["dw_reduce_grouped"])   # (its reduction rides in the grouped reduction launch)
    return d


def _dx_chain(call, dh0, dx, A, A2=None):
    # ``MpgChain`` of dx = dx(node path) + [da | dc] [W1a ; W1c]: one chained layer over the stacked transposed view of fe.net.0.weight.
    # Its three feeds are (A, A2) = (dap, dcp): slab 0 of the partial da and dc [slabs, V, H1] (one chunk, one receiver block: the
    # epilogue of the data-gradient launch); (dadc,): [da | dc] rows as ``mpg_slab_sums`` left them; (da, dc): da rows beside dc rows.
    cfg, pk = call.cfg, call.pk
    return chain_struct(cfg.B * cfg.N, [dict(img=pk.ptr("W1ST"), K=2 * H1, N=cfg.F, resid=dh0[:, H3:H3 + cfg.F], out=dx)],
                        A=A, lda=A.stride(-2), K1=A.shape[-1], A2=A2, lda2=0 if A2 is None else A2.stride(-2), alpha=cfg.alpha, f16=False)


def _data_grad(ctx, call, dh0, bufs, dx):
    # The data-gradient launch of the edge network.  Where the epilogue form covers the call (a whole jet per workgroup) it runs the
    # layer's dx chain behind it, and behind that the node network's input-gradient chain of the layer BELOW, which produced x (its
    # backward then finds its work done: ``ctx.pre``).  Returns which of the routes ran: "with_below", "epilogue" or "plain".
    cfg, lib = call.cfg, _lib.lib()
    e = C.byref(_edge_bwd_desc(call, dh0, bufs))
    tries = []   # (route, the layer's dx chain, the lower layer's FnGrads or None), in the order they are tried
    if dx is not None and cfg.SC == 1 and cfg.N <= 32 and OPTIONS["bwd_epilogue"] and call.sv.es is None:
        cdx = _dx_chain(call, dh0, dx, bufs.dap, bufs.dcp)
        below = _below_chain(ctx.prev_node, dx, cfg.thr, cfg.alpha, cfg.B * cfg.N)
        if below is not None:
            tries.append(("with_below", cdx, below))
        tries.append(("epilogue", cdx, None))   # (the pair is not covered: the layer alone may be)
    for route, cdx, below in tries:
        rc = lib.mpg_edge_bwd_fn(e, C.byref(cdx), None if below is None else C.byref(below.chain), _stream())
        if rc != _lib.MPG_FN_NA:
            check(rc, "mpg_edge_bwd_fn")
            if below is not None:
                ctx.prev_node.pre = FnGradsDone(below, gy_ptr=dx.data_ptr(), keep=dx)
            return route
    check(lib.mpg_edge_bwd(e, _stream()), "mpg_edge_bwd")
    return "plain"


def _slab_sums(dap, dcp):
    # The chunks' partial da and the receiver blocks' partial dc, added slab by slab into [da | dc] rows: one launch (none for one
    # slab each).
    (SC, V, _), RB = dap.shape, dcp.shape[0]
    if SC == 1 and RB == 1:
        return SlabSums(dap[0], dcp[0], None)
    dadc = torch.empty((V, 2 * H1), device=dap.device, dtype=torch.float32)
    check(_lib.lib().mpg_slab_sums(_p(dap), SC, V * H1, _p(dcp), RB, V * H1, _p(dadc), V, H1, _stream()), "mpg_slab_sums")
    return SlabSums(dadc[:, :H1], dadc[:, H1:], dadc)


def _weight_grads(call, gy2, fng, bufs, sums, tg):
    # ``mpg_edge_dw`` (fe.net.1, fe.net.2), then the six dense weight gradients -- fn's three layers and the two halves of fe.net.0
    # (a = W1[:, :F] x + b1, c = W1[:, F:] x) -- as ONE grouped launch.
    # These launches feed nothing before the optimizer: with a side stream set (TrainStep) they are forked off here, behind the
    # data-gradient kernel that produced their inputs, and this stream goes straight on to dx and the layers below.  Same launches,
    # same order per parameter: results are bit-identical.
    sv, cfg, dev, acc, wb = call.sv, call.cfg, call.sv.x2.device, tg.direct, WgradBatch()
    wb.add(fng.dz3, sv.h2, out=tg.V3, bias_out=tg.c3, accumulate=acc)
    wb.add(fng.dz2, sv.h1, out=tg.V2, bias_out=tg.c2, accumulate=acc)
    wb.add(fng.dz1, sv.agg, out=tg.V1, out_col0=0, bias_out=tg.c1, accumulate=acc)
    wb.add(fng.dz1, sv.xf2, out=tg.V1, out_col0=H3, accumulate=acc)
    wb.add(sums.da, sv.x2, out=tg.W1, out_col0=0, bias_out=tg.b1, accumulate=acc)
    wb.add(sums.dc, sv.x2, out=tg.W1, out_col0=cfg.F, accumulate=acc)
    nwg = dw_workgroups(cfg.B * ((cfg.N + 31) // 32) * cfg.N, cfg.N)
    part = torch.empty((nwg, H3 * H2 + H2 * H1 + H3 + H2), device=dev, dtype=torch.float32)   # per-workgroup partials of mpg_edge_dw
    d = _edge_dw_desc(call, fng.dh0, bufs, tg, part)
    st = dev_state(dev)
    side = st.wgrad_stream if (acc and sv.es is None) else None
    if side is not None:
        # wgrad_keep: EVERYTHING a launch on the side stream reads or writes stays referenced until TrainStep joins the stream -- taken
        # from the records that hold those tensors (the saved state, the node network's gradients and their upstream rows, the data
        # gradients and their sums, the partials here and every queued job) rather than listed by hand
        st.wgrad_keep.append((sv, gy2, fng[:4], bufs, sums, part, list(wb.jobs)))
        side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
        check(_lib.lib().mpg_edge_dw(C.byref(d), _stream()), "mpg_edge_dw")
        wb.flush(dw=d if d.defer_reduce else None)


def _edge_backward(ctx, call, gy2, fng, tg, dx):
    # The layer's backward launches: fn's input-gradient chain (unless done), the edge network's data path, then (``tg`` has targets)
    # the weight-gradient pass.  The parked dZ2 lives as long as this call.  Returns (the data-gradient route that ran, the SlabSums, des).
    sv, cfg = call.sv, call.cfg
    need_w = tg.W1 is not None
    bufs = _edge_grad_bufs(call, need_w)
    if fng.chain is not None:
        run_chain(fng.chain)
    route = _data_grad(ctx, call, fng.dh0, bufs, dx)
    sums = _slab_sums(bufs.dap, bufs.dcp)
    if need_w:
        _weight_grads(call, gy2, fng, bufs, sums, tg)
        if sv.es is not None:   # the columns of the edge scalars: sum over receivers of daq
            F, nq = cfg.F, cfg.nq
            dWq = bufs.daq.sum((0, 1))[:nq].t()
            if tg.direct:
                tg.W1[:, 2 * F:2 * F + nq] += dWq
            else:
                tg.W1[:, 2 * F:2 * F + nq] = dWq
    return route, sums, bufs.des


class FusedMPLayerFn(torch.autograd.Function):
    """MPLayer.forward (mpgan/model.py:206-282), default configuration: fully connected, no edge
    features, no conditioning labels; fe = 3 layers [96,160,192], fn = 2 hidden layers + linear."""

    @staticmethod
    def forward(ctx, x, mask, W1, b1, W2, b2, W3, b3, V1, c1, V2, c2, V3, c3, es, xfn, settings):
        """``settings``: an ``MPLayerSettings``.  Its ``nbr`` (from ``knn_sets``) restricts receiver i's senders to its ``num_knn``
        nearest neighbours (``fully_connected=False``, mpgan/model.py:319-381); the mean then divides by ``num_knn`` (:267).

        Its ``handoff`` (a ``LayerHandoff`` or None) couples consecutive layers of a network: ``handoff.below.ac_out`` are this
        layer's layer-1 node terms a | c already computed by the launch that produced ``x`` (then no projection launch here), and
        ``handoff.next`` is the next layer's ``(PackedMPLayer, b1)``: where this call's edge launch runs the node network as
        its epilogue it appends that layer's projection and leaves the result in ``handoff.ac_out``.

        ``es`` [B, N senders, EDGE_SCALARS, N receivers] with ``nq`` live scalars: the edge features / row-tiled conditioning
        columns of the reference (mpgan/model.py:247-253, :297-313), one scalar per edge each; they multiply the columns
        ``W1[:, 2F : 2F + nq]`` (``Z1 = a_i + c_j + sum_q es_q w_q``) and get a gradient.  ``xfn`` [B, N, F + E]: the node
        network's view of the nodes when conditioning columns are appended to it (:270-276); ``V1`` then has E more columns."""
        sum_agg, alpha, p_drop, training, packed, nbr, num_knn, nq, handoff, no_grad, sparse_ok = settings
        _chk(x, "x")
        B, N, F = x.shape
        V, dev, out_f = B * N, x.device, V3.shape[0]
        # ``no_grad``: the caller's torch.is_grad_enabled() was off (train_D's generator call): inside forward() grad mode is
        # always off and needs_input_grad still says what the PARAMETERS want, so without the flag such a call would write
        # everything a backward reads -- sign words, 10 KB of parked fragments per block, agg, h1, h2 -- for nothing
        need_grad = any(ctx.needs_input_grad) and not no_grad
        sparse = bool(sparse_ok and es is None and knn_sparse_route(nbr is not None, nq, N, num_knn))
        if sparse:   # (a sparse layer takes and offers no hand-off, like a spectral-norm layer)
            kp, handoff = knn_plan(B, N, num_knn, need_grad), None   # (raises before any allocation or launch)
        plan = edge_plan(B, N, es=es is not None, mask=mask is not None, need_grad=need_grad and not sparse)   # (raises likewise)
        thr, dscale = drop_params(p_drop) if training else (0, 1.0)
        seed_t = seed_tensor(dev)
        agg_scale = 1.0 if sum_agg else 1.0 / (num_knn if nbr is not None else N)
        cfg = MPLayerCfg(B, N, F, agg_scale, alpha, thr, dscale, next_tag(dev, "mplayer", thr), 1 if sparse else plan.SC, FWD_F16, nq)
        if packed is None or packed.dscale != dscale or packed.f16 != cfg.f16:  # direct callers: pack for this call
            packed = PackedMPLayer((W1, W2, W3, V1, V2, V3), F, out_f, dscale, cfg.f16)
        pk = packed.ensure()
        x2, m1, xf2 = _row_views(x, mask, xfn)
        assert V1.shape[1] == H3 + xf2.shape[1]
        ac = _node_terms(handoff.below if handoff is not None else None, pk, x2, b1, cfg)
        if sparse:
            h1 = torch.empty((V, V1.shape[0]), device=dev, dtype=torch.float32) if need_grad else None
            h2 = torch.empty((V, V2.shape[0]), device=dev, dtype=torch.float32) if need_grad else None
            sv = MPLayerSaved(x2, m1, ac, None, h1, h2, W1, b2, b3, W2, W3, V1, V2, V3, None, nbr, None, None, None, xf2, None)
            y = torch.empty((V, out_f), device=dev, dtype=torch.float32)
            agg, ks = _knn_forward(ctx, MPCall(sv, cfg, pk, seed_t), kp, num_knn, (c1, c2, c3), y, need_grad)
            _leave_offers(ctx, None, x, need_grad)
            ctx.packed, ctx.cfg, ctx.knn = pk, cfg, (kp, num_knn)
            ctx.save_for_backward(*sv._replace(agg=agg), *ks)
            return y.reshape(B, N, out_f)
        ctx.knn = None
        es, wq = _edge_scalar_terms(es, W1, cfg)
        order = jet_order(m1.view(B, N)) if plan.lpt else None
        # (what only a backward reads -- the sign words of the third edge layer, the parked E2, the hidden activations, and agg for
        # fn.net.0's weight gradient -- is not written without one)
        sign3 = torch.empty((B * plan.RB * N * 192,), device=dev, dtype=torch.int32) if need_grad else None
        stE2 = torch.empty((B * plan.RB * N, H2, 32), device=dev, dtype=torch.float16) if need_grad else None
        h1 = torch.empty((V, V1.shape[0]), device=dev, dtype=torch.float32) if need_grad else None
        h2 = torch.empty((V, V2.shape[0]), device=dev, dtype=torch.float32) if need_grad else None
        sv = MPLayerSaved(x2, m1, ac, None, h1, h2, W1, b2, b3, W2, W3, V1, V2, V3, sign3, nbr, stE2, es, wq, xf2, order)   # (agg: below)
        call, y = MPCall(sv, cfg, pk, seed_t), torch.empty((V, out_f), device=dev, dtype=torch.float32)
        aggp = torch.empty((plan.SC, V, H3), device=dev, dtype=torch.float32)
        fn_layers = _fn_fwd_layers(call, (c1, c2, c3), y)
        agg = _fwd_epilogue(call, plan, aggp, fn_layers, handoff) if plan.epilogue else _NOT_COVERED
        if agg is _NOT_COVERED:
            agg = _fwd_two_launches(call, aggp, fn_layers)
        _leave_offers(ctx, handoff, x, need_grad)
        if need_grad and dev_state(dev).sign_tap is not None:
            dev_state(dev).sign_tap.append(dict(B=B, N=N, ac=ac, stE2=stE2, sign3=sign3, h1=h1, h2=h2))
        ctx.packed, ctx.cfg = pk, cfg
        ctx.save_for_backward(*sv._replace(agg=agg))
        return y.reshape(B, N, out_f)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        sv, cfg = mplayer_saved(ctx), ctx.cfg
        (B, N, F), V, dev = cfg[:3], cfg.B * cfg.N, sv.x2.device
        call = MPCall(sv, cfg, ctx.packed, seed_tensor(dev))
        gy2 = gy.reshape(V, -1).contiguous()
        need_x, _, *need_p, _, need_xfn, _ = ctx.needs_input_grad   # (as forward's arguments: x, mask, the twelve parameters, es, xfn, settings)
        # node network fn (mpgan/model.py:279): its input-gradient chain -- already run by the layer above as the epilogue of its
        # data-gradient launch, or launched by _edge_backward
        fng = _taken_fn_grads(ctx, gy2) or _fn_grad_chain(ctx, gy2)
        tg, pg = _grad_targets(call, any(need_p))   # (no parameter wants one in the G step: D's weights get no update there)
        dx = torch.empty((V, F), device=dev, dtype=torch.float32) if need_x else None
        if ctx.knn is not None:
            _knn_backward(ctx, call, knn_saved(ctx), gy2, fng, tg, dx)
            route, des = "knn", None
        else:
            route, sums, des = _edge_backward(ctx, call, gy2, fng, tg, dx)
        if need_x:
            if route == "plain":   # (not done by the data-gradient launch: its own launch)
                run_chain(_dx_chain(call, fng.dh0, dx, *((sums.dadc,) if sums.dadc is not None else (sums.da, sums.dc))))
            dx = dx.reshape(B, N, F)
        dxfn = None
        if need_xfn and fng.dh0.shape[1] > H3 + F:
            # the conditioning columns appended to the node network's input (mpgan/model.py:270-276): their gradient is the
            # tail of dh0; the x columns of xfn are the same nodes as x, whose node-path gradient is already in dx above
            dxfn = torch.cat((torch.zeros((V, F), device=dev, dtype=torch.float32), fng.dh0[:, H3 + F:]), dim=1).reshape(B, N, -1)
        # (parameter gradients already in .grad: autograd gets nothing to accumulate)
        return (dx, None, *pg.slots(), des, dxfn, None)


def _grad_target(t):
    """The .grad buffer a parameter gradient may be added into directly: the leaf's own, or -- for a contiguous
    view of a leaf (a row slice of nn.MultiheadAttention's in_proj_weight / in_proj_bias) -- the matching view of
    the leaf's .grad.  None when there is no such buffer."""
    if t is None:
        return None
    if t.is_leaf:
        return t.grad if (t.grad is not None and t.grad.is_contiguous()) else None
    base = t._base
    if base is None or not base.is_leaf or base.grad is None or not t.is_contiguous() or not base.grad.is_contiguous():
        return None
    return base.grad.as_strided(t.size(), t.stride(), t.storage_offset() - base.storage_offset() + base.grad.storage_offset())


def _deferred_targets(st, params, queue_only=True):
    """The decision step of ``ParamGrads``: may the gradients of ``params`` go into their ``.grad`` buffers?  (the targets in order,
    ``st.deferred_wgrad``) while ``st.grad_into_param`` is on and EVERY parameter has a target, else None.  ``queue_only``: only
    while a backward is collecting as well (a ``WgradBatch`` in ``st.deferred_wgrad``)."""
    if not st.grad_into_param or (queue_only and st.deferred_wgrad is None):
        return None
    targets = [_grad_target(q) for q in params]
    return None if any(t is None for t in targets) else (targets, st.deferred_wgrad)


class ParamGrads:
    """Where the parameter gradients of ONE backward node go: decided here, once, all or nothing over ``params`` (the node's
    parameters in autograd's order; ``wanted``: which of them get a gradient; ``st``: the ``DeviceState``).
      queued    ``st.grad_into_param``, a collecting ``st.deferred_wgrad`` and a ``_grad_target`` for EVERY wanted parameter (a
                wanted None has none): ``gemm`` and ``colsum`` add jobs to that ``WgradBatch``, whose grouped launch adds into
                .grad at ``flush()``;
      direct    the flag and every target: a kernel that forms the gradients itself adds into .grad (``written``);
      returned  otherwise: fresh tensors, handed to autograd.
    ``eligible``: what else the node needs to leave the returned route.  ``slots()`` is the node's answer to autograd: None
    wherever the gradient went into .grad, so none can be returned and accumulated as well.
    One per node, but for ``FusedMABFn``: its six GEMM-shaped gradients share one, while each norm parameter and the seed row
    decide alone, as they always have (``_colsum_grad``: one helper of one parameter each)."""

    __slots__ = ("wanted", "out", "targets", "batch")

    def __init__(self, st, params, wanted, eligible=True):
        self.wanted, self.out = wanted, [None] * len(params)
        self.targets = self.batch = None
        found = _deferred_targets(st, [q for q, w in zip(params, wanted) if w], queue_only=False) if (eligible and any(wanted)) else None
        if found is not None:
            tg = iter(found[0])
            self.targets, self.batch = [next(tg) if w else None for w in wanted], found[1]

    def slots(self):
        return tuple(self.out)

    def _give(self, i, t):   # (row blocks of one parameter -- cross-attention's Win[:E] / Win[E:] -- one under the other)
        self.out[i] = t if self.out[i] is None else torch.cat([self.out[i], t], 0)

    def gemm(self, iw, ib, dy, x, *, rows=None, col0=0):
        """dW[rows, col0:col0+K] = dy^T x for parameter ``iw`` and its column sums for the bias ``ib`` (or None), as far as
        they are wanted: a job of the batch when queued, else ``linear_bwd_weight`` into fresh tensors; a bias alone is summed
        here and returned on every route (there is no GEMM for it to ride in).  ``col0`` (``WgradBatch.add``'s ``out_col0``) is
        for the queued route only and no site passes it yet; ``out_scale`` is not offered: no site scales."""
        want_b = ib is not None and self.wanted[ib]
        if not self.wanted[iw]:
            if want_b:
                self._give(ib, dy.sum(0))
        elif self.batch is not None:
            W, b = self.targets[iw], self.targets[ib] if want_b else None
            self.batch.add(dy, x, out=W if rows is None else W[rows], out_col0=col0,
                           bias_out=b if (b is None or rows is None) else b[rows], accumulate=True)
        else:
            assert col0 == 0, "a column block of dW is formed on the queued route only"
            db = torch.empty(dy.shape[1], device=dy.device, dtype=torch.float32) if want_b else None
            self._give(iw, linear_bwd_weight(dy, x, bias_out=db))
            if want_b:
                self._give(ib, db)

    def colsum(self, i, rows):
        """The column sums of ``rows`` [M, E] for the vector parameter ``i``: queued, a bias-sum job (its one-column GEMM goes
        into a throw-away ``out``); else summed here."""
        if self.wanted[i] and self.batch is not None:
            self.batch.add(rows, rows[:, :1], out=rows.new_empty((rows.shape[1], 1)), bias_out=self.targets[i].reshape(-1), accumulate=True)
        elif self.wanted[i]:
            self.out[i] = rows.sum(0)

    def written(self, fresh, scratch=False):
        """For a kernel that writes the gradients itself: (the tensors it writes, its ``accumulate`` flag) -- the .grad targets and
        1, what ``fresh()`` allocates and 0, or Nones and 0 when nothing is wanted.  ``scratch``: the launch needs its buffers
        even then (``mpg_batchnorm_bwd``): ``fresh()`` as well, but autograd still gets Nones."""
        if self.targets is not None:
            return self.targets, 1
        if any(self.wanted):
            self.out = list(fresh())
            return self.out, 0
        return (list(fresh()) if scratch else self.out), 0


class FusedLinearFn(torch.autograd.Function):
    """Linear -> [LeakyReLU] -> [Dropout] (one LinearNet layer; mpgan/model.py:77-83), optionally ``+ resid`` in the
    same launch (MAB's residual connections, gapt/model.py:131-137; only for a layer without activation)."""

    @staticmethod
    def forward(ctx, x, W, b, act, alpha, p_drop, training, resid=None):
        _chk(x, "x")
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        if x2.stride(1) != 1 or x2.stride(0) < shp[-1]:   # (rows of any stride are fine -- a column slice of wider rows, D's x[..., :-1] -- only unit column stride matters)
            x2 = x2.contiguous()
        thr, dscale = drop_params(p_drop) if training else (0, 1.0)
        seed_t = seed_tensor(x.device)
        tag = next_tag(x.device, "linear", thr)
        if resid is not None and act:  # (the backward reads the activation's sign off the saved output)
            raise NotImplementedError("FusedLinearFn: a fused residual needs a layer without activation")
        r2 = None if resid is None else resid.reshape(-1, W.shape[0]).contiguous()
        y = linear_fwd(x2, W, b, act=act, alpha=alpha, drop=(seed_t, tag + TAG_GENERIC, thr, dscale) if thr else None,
                       resid=r2)
        ctx.has_resid = resid is not None
        ctx.save_for_backward(x2, W, y)
        ctx.wparam, ctx.bias = W, b  # (only their .grad buffers are touched, by the deferred weight-gradient path)
        ctx.cfg = (shp, act, alpha, thr, dscale, tag, b is not None)
        return y.reshape(*shp[:-1], W.shape[0])

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x2, W, y = ctx.saved_tensors
        shp, act, alpha, thr, dscale, tag, _ = ctx.cfg
        g2 = gy.reshape(-1, W.shape[0]).contiguous()
        if act or thr:
            g2 = gate(g2, y, gate_act=act, alpha=alpha, seed_t=seed_tensor(g2.device), tag=tag + TAG_GENERIC,
                      thr=thr, scale=dscale)
        # (TrainStep: dW (+ db) queued for the grouped launch at the end of the backward, which adds into .grad)
        pg = ParamGrads(dev_state(g2.device), (ctx.wparam, ctx.bias), ctx.needs_input_grad[1:3])
        pg.gemm(0, 1, g2, x2)
        dx = linear_bwd_data(g2, W).reshape(shp) if ctx.needs_input_grad[0] else None
        return dx, *pg.slots(), None, None, None, None, (gy if ctx.has_resid else None)


class MatMulFn(torch.autograd.Function):
    """C = A B^T ("nt"), A B ("nn") or A^T B ("tn") on ``mpg_gemm`` -- with a backward that is written in terms of
    ``MatMulFn`` itself, so that it can be differentiated again, to any order.  The three forms are closed under
    differentiation:  nt: dA = G B (nn), dB = G^T A (tn);  nn: dA = G B^T (nt), dB = A^T G (tn);  tn: dA = B G^T (nt),
    dB = A G (nn).  This is the product the double-backward route is made of (``LinearNet._forward_dd``): the gradient
    penalty (train.py:286-324) differentiates D's input gradient once more, which the fused kernels
    (``once_differentiable``) decline."""

    @staticmethod
    def forward(ctx, A, B, form):
        _chk(A, "A"); _chk(B, "B")
        A, B = A.contiguous(), B.contiguous()
        ctx.form = form
        ctx.save_for_backward(A, B)
        if form == "nt":   # (bf16 hi/lo like the other two forms: gradients of any magnitude pass through all three)
            return linear_fwd(A, B, None, f16=False)
        if form == "nn":
            return linear_bwd_data(A, B)
        if form == "tn":
            return linear_bwd_weight(A, B)
        raise ValueError(f"MatMulFn: form must be nt / nn / tn, got {form!r}")

    @staticmethod
    def backward(ctx, G):
        A, B = ctx.saved_tensors
        nA, nB = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        mm = MatMulFn.apply
        if ctx.form == "nt":
            return (mm(G, B, "nn") if nA else None), (mm(G, A, "tn") if nB else None), None
        if ctx.form == "nn":
            return (mm(G, B, "nt") if nA else None), (mm(A, G, "tn") if nB else None), None
        return (mm(B, G, "nt") if nA else None), (mm(A, G, "nn") if nB else None), None


class double_backward_route:
    """``with ops.double_backward_route(device):`` -- modules called inside take the route that can be differentiated
    twice: every product a ``MatMulFn``, everything elementwise plain ATen (whose backward formulas are differentiable
    themselves), the edge matrix materialised as the reference builds it.  First-order-only pieces (the fused
    message-passing and attention kernels, batch norm) are not used there; a configuration that needs one raises."""

    def __init__(self, device="cuda"):
        self.state = dev_state(device)

    def __enter__(self):
        self.prev, self.state.double_backward = self.state.double_backward, True
        return self

    def __exit__(self, *exc):
        self.state.double_backward = self.prev
        return False


def double_backward_on(device) -> bool:
    return dev_state(device).double_backward


# ---- a per-particle layer and the pooling over a jet's particles in one launch (ext_models.rGAND / PointNetMixD) ------------------
POINT_POOL_MAX = (_lib.POINT_POOL_MAX_N, _lib.POINT_POOL_MAX_K, _lib.POINT_POOL_MAX_C)
POINT_POOL_MODES = {1: "max", 2: "mean", 3: "max | mean"}


def point_pool_route(N, K, C, double_backward, options=None) -> bool:
    """Does a layer-and-pool call run on ``PointPoolFn`` (mpg_point_pool_fwd / _bwd)?  With the option on
    (``OPTIONS["point_pool"]``), outside the double-backward route (the launch pair is once differentiable) and inside the kernel's
    limits: 1 <= N <= 160 particles, 1 <= K <= 256 input columns, 1 <= C <= 1024 channels.  Host only."""
    opt = OPTIONS if options is None else options
    if not opt.get("point_pool") or double_backward:
        return False
    return all(1 <= int(v) <= m for v, m in zip((N, K, C), POINT_POOL_MAX))


def _point_pool_desc(x2, W, b, B, N, act, alpha, mode):
    e = _lib.MpgPointPool()
    e.x, e.ldx, e.W, e.ldw, e.bias = _p(x2), x2.stride(0), _p(W), W.stride(0), _p(b)
    e.B, e.N, e.K, e.C = B, N, W.shape[1], W.shape[0]
    e.act, e.alpha, e.mode, e.f16 = int(act), alpha, mode, 1
    return e


class PointPoolFn(torch.autograd.Function):
    """pooled [B, C or 2 C] = max and / or mean over the N particles of each jet of  act(x W^T + b),  x [B N, K]: the last point
    layer of rGAND (ext_models.py:70-71) and PointNetMixD (:203-206) with its pooling, one launch; the [B N, C] activation is not
    written.  ``mode``: 1 max, 2 mean, 3 cat((max, mean), 1).  The backward expands the cotangent into dz [B N, C] (one element-wise
    launch on the argmax rows and sign bits the forward kept), dx = dz W on ``linear_bwd_data`` and dW, db through ``ParamGrads`` as
    ``FusedLinearFn``'s.  Nothing is read back: capturable."""

    @staticmethod
    def forward(ctx, x, W, b, B, N, act, alpha, mode, grad_mode=True):
        _chk(x, "x"); _chk(W, "W")
        if mode not in POINT_POOL_MODES:
            raise ValueError(f"point_pool: mode must be 1 (max), 2 (mean) or 3 (max | mean), got {mode!r}")
        x2 = x.reshape(B * N, W.shape[1])
        if x2.stride(1) != 1 or x2.stride(0) < W.shape[1]:
            x2 = x2.contiguous()
        Wc = W if W.stride(1) == 1 else W.contiguous()
        Cn = W.shape[0]
        dev = x.device
        # (``needs_input_grad`` says what the inputs ask for whatever the grad mode: under ``no_grad`` nothing is kept)
        need = grad_mode and any(ctx.needs_input_grad[:3])
        argmax = torch.empty((B, Cn), device=dev, dtype=torch.int32) if (need and mode & 1) else None
        neg = torch.empty((B * N, (Cn + 31) // 32), device=dev, dtype=torch.int32) if (need and act) else None
        pooled = point_pool_launch(x2, Wc, b, B, N, act=act, alpha=alpha, mode=mode, argmax=argmax, neg=neg)
        ctx.save_for_backward(x2, Wc, argmax, neg)
        ctx.wparam, ctx.bias = W, b
        ctx.cfg = (x.shape, B, N, act, alpha, mode)
        return pooled

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x2, W, argmax, neg = ctx.saved_tensors
        shp, B, N, act, alpha, mode = ctx.cfg
        g2 = g if (g.stride(1) == 1 and g.stride(0) >= g.shape[1]) else g.contiguous()
        dz = point_pool_bwd_launch(g2, argmax, neg, B, N, W.shape[0], act=act, alpha=alpha, mode=mode)
        pg = ParamGrads(dev_state(g.device), (ctx.wparam, ctx.bias), ctx.needs_input_grad[1:3])
        pg.gemm(0, 1, dz, x2)
        dx = linear_bwd_data(dz, W).reshape(shp) if ctx.needs_input_grad[0] else None
        return dx, *pg.slots(), None, None, None, None, None, None


def point_pool(x, W, b, B, N, *, act=True, alpha=0.2, mode=1):
    """``PointPoolFn``: [B, C] (mode 1: max; 2: mean) or [B, 2 C] (mode 3: max | mean) of act(x W^T + b) over each jet's N rows."""
    return PointPoolFn.apply(x, W, b, B, N, bool(act), float(alpha), int(mode), torch.is_grad_enabled())


def point_pool_launch(x2, W, b, B, N, *, act, alpha, mode, argmax=None, neg=None):
    """The forward launch on caller-owned by-product buffers (``argmax`` int32 [B, C], ``neg`` int32 [B N, ceil(C / 32)], or None)."""
    Cn = W.shape[0]
    pooled = torch.empty((B, Cn * (2 if mode == 3 else 1)), device=x2.device, dtype=torch.float32)
    e = _point_pool_desc(x2, W, b, B, N, act, alpha, mode)
    e.pooled, e.ld_pooled, e.argmax, e.neg = _p(pooled), pooled.stride(0), _p(argmax), _p(neg)
    check(_lib.lib().mpg_point_pool_fwd(C.byref(e), _stream()), "mpg_point_pool_fwd")
    return pooled


def point_pool_bwd_launch(g, argmax, neg, B, N, Cn, *, act, alpha, mode):
    """The backward launch alone: dz [B N, C] of the cotangent ``g`` of pooled."""
    dz = torch.empty((B * N, Cn), device=g.device, dtype=torch.float32)
    e = _lib.MpgPointPool()
    e.B, e.N, e.K, e.C, e.act, e.alpha, e.mode, e.f16 = B, N, 1, Cn, int(act), alpha, mode, 1
    e.argmax, e.neg = _p(argmax), _p(neg)
    e.gpooled, e.ld_gpooled, e.dz, e.ld_dz = _p(g), g.stride(0), _p(dz), dz.stride(0)
    check(_lib.lib().mpg_point_pool_bwd(C.byref(e), _stream()), "mpg_point_pool_bwd")
    return dz


# ---- one TreeGCN layer of the TreeGAN generator in one launch per direction (ext_models.TreeGANG) ---------------------------------
TREE_GCN_MAX = (_lib.TREE_GCN_MAX_LEVELS, _lib.TREE_GCN_MAX_WIDTH, _lib.TREE_GCN_MAX_BRANCH, _lib.TREE_GCN_MAX_NODES)


def tree_gcn_route(features, degrees, depth, double_backward, options=None) -> bool:
    """Does layer ``depth`` of a tree with these ``features`` / ``degrees`` run on ``TreeGcnFn`` (mpg_tree_gcn_fwd / _bwd)?  With
    the option on (``OPTIONS["tree_gcn"]``), outside the double-backward route (the launch pair is once differentiable) and inside
    the kernel's limits: depth < 8, every width of levels 0 .. depth + 1 in 1 .. 128, degree * in <= 256, nodes * degree <= 160,
    every degree >= 1.  Host only."""
    opt = OPTIONS if options is None else options
    if not opt.get("tree_gcn") or double_backward:
        return False
    levels, width, branch, nodes = TREE_GCN_MAX
    d = int(depth)
    if not 0 <= d < levels or len(features) < d + 2 or len(degrees) < d + 1:
        return False
    if any(not 1 <= int(f) <= width for f in features[:d + 2]) or any(int(g) < 1 for g in degrees[:d + 1]):
        return False
    P = 1
    for g in degrees[:d]:
        P *= int(g)
    return int(degrees[d]) * int(features[d]) <= branch and P * int(degrees[d]) <= nodes


def _tree_gcn_desc(shapes, W_branch, Wc, act, alpha):
    """``shapes``: (nodes, width) of the levels 0 .. d.  The sizes both directions check."""
    e = _lib.MpgTreeGcn()
    for i, (nodes, width) in enumerate(shapes):
        e.nodes[i], e.width[i] = nodes, width
    e.d, e.P = len(shapes) - 1, shapes[-1][0]
    setattr(e, "in", Wc.shape[1])
    e.out, e.g = Wc.shape[0], W_branch.shape[2] // Wc.shape[1]
    e.W_branch, e.Wc, e.act, e.alpha = _p(W_branch), _p(Wc), int(act), alpha
    return e


def tree_gcn_launch(levels, W_roots, W_branch, Wc, bias, *, act, alpha, y=None, u=None):
    """The forward launch: tree[d + 1] as rows [B P g, out] from the contiguous levels 0 .. d ([B, P_i, width_i]), the root weights
    ([out, width_i]), W_branch [P, in, g in], Wc [out, in] and bias [g out] (or None).  ``y`` / ``u``: caller-owned row views (unit
    column stride) to write into; ``u`` None: u is not written."""
    B, P = levels[-1].shape[:2]
    g, out = W_branch.shape[2] // Wc.shape[1], Wc.shape[0]
    if y is None:
        y = torch.empty((B * P * g, out), device=Wc.device, dtype=torch.float32)
    e = _tree_gcn_desc([t.shape[1:] for t in levels], W_branch, Wc, act, alpha)
    for i, (t, W) in enumerate(zip(levels, W_roots)):
        e.level[i], e.W_root[i] = t.data_ptr(), W.data_ptr()
    e.B, e.bias = B, _p(bias)
    e.y, e.ld_y, e.u, e.ld_u = _p(y), y.stride(0), _p(u), 0 if u is None else u.stride(0)
    check(_lib.lib().mpg_tree_gcn_fwd(C.byref(e), _stream()), "mpg_tree_gcn_fwd")
    return y


def tree_gcn_bwd_launch(dy, y, u, shapes, W_branch, Wc, *, act, alpha, need_dx=True):
    """The backward launch alone, on rows: (dz [B P g, out], S [B P, out], du [B P g, in], dx [B P, in] or None) of the cotangent
    ``dy`` [B P g, out]; ``y`` the stored output (read with ``act``), ``u`` the stored branch activation."""
    P, inn, out = shapes[-1][0], Wc.shape[1], Wc.shape[0]
    g = W_branch.shape[2] // inn
    B = dy.shape[0] // (P * g)
    new = lambda *s: torch.empty(s, device=dy.device, dtype=torch.float32)
    dz, S, du, dx = new(B * P * g, out), new(B * P, out), new(B * P * g, inn), (new(B * P, inn) if need_dx else None)
    e = _tree_gcn_desc(shapes, W_branch, Wc, act, alpha)
    e.B = B
    e.y, e.ld_y, e.u, e.ld_u = _p(y), 0 if y is None else y.stride(0), _p(u), u.stride(0)
    e.dy, e.ld_dy, e.dz, e.ld_dz = _p(dy), dy.stride(0), _p(dz), dz.stride(0)
    e.S, e.du, e.dx = _p(S), _p(du), _p(dx)
    check(_lib.lib().mpg_tree_gcn_bwd(C.byref(e), _stream()), "mpg_tree_gcn_bwd")
    return dz, S, du, dx


class TreeGcnFn(torch.autograd.Function):
    """tree[d + 1] [B, P g, out] of one TreeGCN layer (ext_models.py:254-282, ``upsample``) from the levels 0 .. d: the ancestor
    sum, the per-node branch product, its LeakyReLU, the loop product, bias and activation in one launch.  W_loop's two bias-free
    Linears have nothing between them, so their product Wc = W_loop.1 W_loop.0 [out, in] (one ``mpg_gemm`` in front of the launch,
    every forward: nothing is cached on the host, the op stays right under graph replay with weights updated in place) gives the
    same forward, and the [rows, in support] activation is never formed; the gradients of both factors follow from M = dz^T u as
    dW_loop.0 = W_loop.1^T M, dW_loop.1 = M W_loop.0^T.  Saved: the levels, u [B P g, in] and (with ``act``) the output.
    Arguments behind the flags: W_branch, W_loop.0, W_loop.1, bias ([1, g, out] or None: the last layer's bias is not read and
    gets no gradient), the d + 1 levels, the d + 1 root weights.  Nothing is read back: capturable."""

    @staticmethod
    def forward(ctx, act, alpha, grad_mode, W_branch, W0, W1, bias, *rest):
        n = len(rest) // 2
        for t in rest + (W_branch, W0, W1):
            _chk(t, "tree_gcn")
        levels, roots = [t.contiguous() for t in rest[:n]], [t.contiguous() for t in rest[n:]]
        Wb, W0c, W1c = W_branch.contiguous(), W0.contiguous(), W1.contiguous()
        Wc = linear_bwd_data(W1c, W0c)   # [out, in] = W_loop.1 W_loop.0
        B, P, inn = levels[-1].shape
        g, out = Wb.shape[2] // inn, W1.shape[0]
        # (``needs_input_grad`` says what the inputs ask for whatever the grad mode: under ``no_grad`` nothing is kept)
        need = grad_mode and any(ctx.needs_input_grad)
        u = torch.empty((B * P * g, inn), device=Wc.device, dtype=torch.float32) if need else None
        y = tree_gcn_launch(levels, roots, Wb, Wc, None if bias is None else bias.reshape(-1), act=act, alpha=alpha, u=u)
        ctx.save_for_backward(y if act else None, u, Wc, Wb, W0c, W1c, *levels, *roots)
        ctx.params = (W_branch, W0, W1, bias) + tuple(rest[n:])   # (only their .grad buffers are touched: ``ParamGrads``)
        ctx.cfg = (act, alpha, n, g)
        return y.view(B, P * g, out)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        y, u, Wc, Wb, W0, W1, *rest = ctx.saved_tensors
        act, alpha, n, g = ctx.cfg
        levels, roots = rest[:n], rest[n:]
        B, P, inn = levels[-1].shape
        out = Wc.shape[0]
        need_lv = ctx.needs_input_grad[7:7 + n]
        dz, S, du, dx = tree_gcn_bwd_launch(gy.reshape(B * P * g, out).contiguous(), y, u, [t.shape[1:] for t in levels], Wb, Wc,
                                            act=act, alpha=alpha, need_dx=need_lv[-1])
        pg = ParamGrads(dev_state(gy.device), ctx.params, ctx.needs_input_grad[3:7] + ctx.needs_input_grad[7 + n:])
        if pg.wanted[3]:
            pg.colsum(3, dz.view(B * P, g * out))
            if pg.out[3] is not None:
                pg.out[3] = pg.out[3].view(1, g, out)
        # every GEMM-shaped gradient of the layer is one job: of the collecting batch when queued (``pg.gemm``), else of ONE grouped
        # launch of this node's own into fresh tensors
        own = WgradBatch()

        def wgrad(i, dy, x, rows=None):
            if not pg.wanted[i]:
                return
            if pg.batch is not None:
                return pg.gemm(i, None, dy, x, rows=rows)
            if pg.out[i] is None:
                pg.out[i] = torch.empty_like(ctx.params[i], memory_format=torch.contiguous_format)
            own.add(dy, x, out=pg.out[i] if rows is None else pg.out[i][rows])

        if pg.wanted[1] or pg.wanted[2]:
            M = linear_bwd_weight(dz, u)                             # [out, in]
            wgrad(1, W1, M)                                          # W_loop.1^T M
            if pg.wanted[2]:
                wgrad(2, M.t().contiguous(), W0.t().contiguous())    # M W_loop.0^T
        du3 = du.view(B, P, g * inn)
        for p in range(P if pg.wanted[0] else 0):                    # dW_branch[p] = tree[d][:, p]^T du[:, p]
            wgrad(0, levels[-1][:, p], du3[:, p], rows=p)
        # the root terms, from the finest level up: S_i sums S over the descendants of a level-i node (node order)
        dlev, Si = [None] * n, S.view(B, P, out)
        for i in reversed(range(n)):
            Pi = levels[i].shape[1]
            if Si.shape[1] != Pi:
                Si = Si.view(B, Pi, Si.shape[1] // Pi, out).sum(2)
            rows = Si.reshape(B * Pi, out)
            wgrad(4 + i, rows, levels[i].view(B * Pi, -1))
            if need_lv[i]:
                if i == n - 1:
                    dlev[i] = linear_bwd_data(rows, roots[i], out=dx, accumulate=True).view(B, P, inn)
                else:
                    dlev[i] = linear_bwd_data(rows, roots[i]).view(B, Pi, -1)
        own.flush()
        slots = pg.slots()
        return (None, None, None, *slots[:4], *dlev, *slots[4:])


def tree_gcn(levels, W_roots, W_branch, W0, W1, bias, *, act=True, alpha=0.2):
    """``TreeGcnFn``: tree[d + 1] [B, P g, out] from the levels 0 .. d, their root weights, W_branch [P, in, g in], W_loop's two
    weights and bias [1, g, out] (None: no bias)."""
    return TreeGcnFn.apply(bool(act), float(alpha), torch.is_grad_enabled(), W_branch, W0, W1, bias, *levels, *W_roots)


# ---- NNConv (edge-conditioned convolution, mean aggregation) of the GraphCNN-GAN generator in one launch per direction ---------------
NNCONV_MAX = (_lib.NNCONV_MAX_N, _lib.NNCONV_MAX_C, _lib.NNCONV_MAX_C)


def nnconv_route(N, Cin, Cout, double_backward, options=None) -> bool:
    """Does an NNConv call run on ``NNConvFn`` (mpg_nnconv_fwd / _bwd)?  With the option on (``OPTIONS["nnconv"]``), outside the
    double-backward route (the launch pair is once differentiable) and inside the kernel's limits: 1 <= N <= 160 nodes per jet,
    1 <= Cin, Cout <= 64.  Host only."""
    opt = OPTIONS if options is None else options
    if not opt.get("nnconv") or double_backward:
        return False
    return all(1 <= int(v) <= m for v, m in zip((N, Cin, Cout), NNCONV_MAX))


def _nnconv_desc(x2, nbr, nn_weight, nn_bias, root, B, N):
    e = _lib.MpgNNConv()
    e.x, e.ld_x, e.nbr = _p(x2), x2.stride(0), C.c_void_p(nbr.data_ptr())
    e.nn_weight, e.nn_bias, e.root = _p(nn_weight), _p(nn_bias), _p(root)
    e.B, e.N, e.Cin, e.Cout = B, N, root.shape[0], root.shape[1]
    return e


def nnconv_launch(x2, nbr, nn_weight, nn_bias, root, bias, B, N, *, y=None, pm=None):
    """The forward launch: y [B N, Cout] from the rows x2 [B N, Cin] (unit column stride), the neighbour words ``nbr`` of
    ``knn_sets`` ([B N, ceil(N / 32)] int32) and the four contiguous parameters.  ``y``: a caller-owned row view to write into;
    ``pm``: a contiguous [B N, Cin (Cin + 1)] array that receives [P | m], or None: not written."""
    Cin, Cout = root.shape
    if y is None:
        y = torch.empty((B * N, Cout), device=x2.device, dtype=torch.float32)
    e = _nnconv_desc(x2, nbr, nn_weight, nn_bias, root, B, N)
    e.bias, e.y, e.ld_y, e.pm = _p(bias), _p(y), y.stride(0), _p(pm)
    check(_lib.lib().mpg_nnconv_fwd(C.byref(e), _stream()), "mpg_nnconv_fwd")
    return y


def nnconv_bwd_launch(dy, x2, nbr, pm, nn_weight, nn_bias, root, B, N, *, dx=None, g=None):
    """The backward launch alone: dx [B N, Cin] (all three shares) of the cotangent rows ``dy`` [B N, Cout] from the parked
    ``pm``; ``g``: the [B N, Cin (Cin + 1)] workspace that receives [G | dm] (allocated when None).  ``dx``: a caller-owned row
    view to write into."""
    Cin = root.shape[0]
    if dx is None:
        dx = torch.empty((B * N, Cin), device=dy.device, dtype=torch.float32)
    if g is None:
        g = torch.empty((B * N, Cin * (Cin + 1)), device=dy.device, dtype=torch.float32)
    e = _nnconv_desc(x2, nbr, nn_weight, nn_bias, root, B, N)
    e.pm, e.dy, e.ld_dy, e.g, e.dx, e.ld_dx = _p(pm), _p(dy), dy.stride(0), _p(g), _p(dx), dx.stride(0)
    check(_lib.lib().mpg_nnconv_bwd(C.byref(e), _stream()), "mpg_nnconv_bwd")
    return dx


class NNConvFn(torch.autograd.Function):
    """y [B N, Cout] of PyG's NNConv (aggr "mean", root weight, bias; ext_models.py:94-121) on the neighbour sets ``nbr`` of
    ``knn_sets``, edge attribute x_j - x_i, in the factorised form of csrc/nnconv.hip: no weight matrix per edge, forward or
    backward.  With a gradient wanted the forward parks [P | m] [B N, Cin (Cin + 1)]; the backward launch writes dx, and the
    four parameter gradients are GEMM jobs through ``ParamGrads`` that land in the parameters' own layouts (nn.weight's row block
    c Cout .. (c + 1) Cout from columns c Cin .. of P: one job per c).  The raw parameters are read by every launch: nothing is
    cached on the host, the op stays right under graph replay with weights updated in place.  ``nbr`` carries no gradient.
    Nothing is read back: capturable."""

    @staticmethod
    def forward(ctx, x, nbr, nn_weight, nn_bias, root, bias, B, N, grad_mode=True):
        for t in (x, nn_weight, nn_bias, root, bias):
            _chk(t, "nnconv")
        Cin, Cout = root.shape
        x2 = x.reshape(B * N, Cin)
        if x2.stride(1) != 1 or x2.stride(0) < Cin:
            x2 = x2.contiguous()
        Wn, bn, rt, bs = nn_weight.contiguous(), nn_bias.contiguous(), root.contiguous(), bias.contiguous()
        nbr = nbr.contiguous()
        # (``needs_input_grad`` says what the inputs ask for whatever the grad mode: under ``no_grad`` nothing is kept)
        need = grad_mode and any(ctx.needs_input_grad)
        pm = torch.empty((B * N, Cin * (Cin + 1)), device=x.device, dtype=torch.float32) if need else None
        y = nnconv_launch(x2, nbr, Wn, bn, rt, bs, B, N, pm=pm)
        ctx.save_for_backward(x2, nbr, pm, Wn, bn, rt)
        ctx.params = (nn_weight, nn_bias, root, bias)   # (only their .grad buffers are touched: ``ParamGrads``)
        ctx.cfg = (x.shape, B, N)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x2, nbr, pm, Wn, bn, rt = ctx.saved_tensors
        shp, B, N = ctx.cfg
        Cin, Cout = rt.shape
        dy = gy if (gy.stride(1) == 1 and gy.stride(0) >= Cout) else gy.contiguous()
        dx = nnconv_bwd_launch(dy, x2, nbr, pm, Wn, bn, rt, B, N).reshape(shp) if ctx.needs_input_grad[0] else None
        pg = ParamGrads(dev_state(gy.device), ctx.params, ctx.needs_input_grad[2:6])
        pg.colsum(3, dy)
        own = WgradBatch()

        def wgrad(i, a, b, view, rows=None):
            """``view(target)[rows] = a^T b``: a job of the collecting batch when queued, else of this node's own grouped launch"""
            if pg.batch is not None:
                out = view(pg.targets[i])
                return pg.batch.add(a, b, out=out if rows is None else out[rows], accumulate=True)
            if pg.out[i] is None:
                pg.out[i] = torch.empty_like(ctx.params[i], memory_format=torch.contiguous_format)
            out = view(pg.out[i])
            own.add(a, b, out=out if rows is None else out[rows])

        if pg.wanted[0]:     # d nn.weight[c Cout + o, d] = sum_i dy_i[o] P_i[c,d]
            for c in range(Cin):
                wgrad(0, dy, pm[:, c * Cin:(c + 1) * Cin], lambda t: t.view(Cin, Cout, Cin), rows=c)
        if pg.wanted[1]:     # d nn.bias[c Cout + o] = sum_i m_i[c] dy_i[o]
            wgrad(1, pm[:, Cin * Cin:], dy, lambda t: t.view(Cin, Cout))
        if pg.wanted[2]:     # d root = x^T dy
            wgrad(2, x2, dy, lambda t: t)
        own.flush()
        return (dx, None, *pg.slots(), None, None, None)


def _nbr_dense(nbr, B, N):
    """The neighbour words as a 0 / 1 float adjacency [B, N, N] (receiver, sender) and the rows' counts [B, N]; on the device."""
    W = nbr.shape[-1]
    bits = (nbr.view(B, N, W, 1) >> torch.arange(32, device=nbr.device, dtype=torch.int32)) & 1
    adj = bits.reshape(B, N, W * 32)[:, :, :N].to(torch.float32)
    return adj, adj.sum(2)


def nnconv_literal(x, adj, nn_weight, nn_bias, root, bias, B, N, k, *, double_backward=False):
    """The un-fused route, PyG's layer as written: gather the ``k`` listed neighbours of every node (``adj`` [B, N, N], 0 / 1; a
    row with fewer takes part with weight 0 in the slots left over), a weight matrix per edge from the Linear on x_j - x_i, the
    per-edge product, the mean over the listed neighbours, root and bias.  Every Linear a ``FusedLinearFn`` (``MatMulFn`` with
    ``double_backward``: twice differentiable), the rest ATen.  CPU tensors: plain torch."""
    Cin, Cout = root.shape
    x3 = x.reshape(B, N, Cin)
    val, idx = adj.topk(k, dim=2)                                     # [B, N, k]: the set bits first
    cnt = adj.sum(2).clamp(min=1.0)
    xj = x3.gather(1, idx.reshape(B, N * k, 1).expand(B, N * k, Cin)).reshape(B, N, k, Cin)
    ea = (xj - x3.unsqueeze(2)).reshape(B * N * k, Cin)
    if not x.is_cuda:
        We = torch.nn.functional.linear(ea, nn_weight, nn_bias)
        own = x3.reshape(B * N, Cin) @ root
    elif double_backward:
        We = MatMulFn.apply(ea, nn_weight, "nt") + nn_bias
        own = MatMulFn.apply(x3.reshape(B * N, Cin), root, "nn")
    else:
        We = FusedLinearFn.apply(ea, nn_weight, nn_bias, False, 0.2, 0.0, False, None)
        own = MatMulFn.apply(x3.reshape(B * N, Cin), root, "nn")
    msg = torch.bmm(xj.reshape(B * N * k, 1, Cin), We.view(B * N * k, Cin, Cout)).view(B, N, k, Cout)
    agg = (msg * val.unsqueeze(3).to(msg.dtype)).sum(2) / cnt.unsqueeze(2).to(msg.dtype)
    return agg.reshape(B * N, Cout) + own + bias


def nnconv(x, nbr, nn_weight, nn_bias, root, bias, *, k=None):
    """NNConv (mean aggregation, root weight, bias) of the rows ``x`` [B, N, Cin] on the neighbour words ``nbr`` [B N, ceil(N / 32)]
    of ``knn_sets``: [B N, Cout].  ``NNConvFn`` where ``nnconv_route`` says yes, else ``nnconv_literal`` (``k``: the largest
    number of neighbours a row lists; None: read back from the words)."""
    B, N, Cin = x.shape
    dd = double_backward_on(x.device)
    if nnconv_route(N, Cin, root.shape[1], dd):
        return NNConvFn.apply(x, nbr, nn_weight, nn_bias, root, bias, B, N, torch.is_grad_enabled())
    adj, cnt = _nbr_dense(nbr, B, N)
    if k is None:
        k = int(cnt.max())
    return nnconv_literal(x, adj, nn_weight, nn_bias, root, bias, B, N, max(1, min(int(k), N)), double_backward=dd)


# ---- PCGAN's set encoder: equivariant stack and max over particles in one forward-only launch (ext_models.G_inv_Tanh / G_inv) ------
SET_ENC_MAX = (_lib.SET_ENC_MAX_N, _lib.SET_ENC_MAX_D, _lib.SET_ENC_MAX_LAYERS)
SET_ENC_POOLS = {"max1": 1, "max": 2, "mean": 3}      # PermEqui1_max, PermEqui2_max, PermEqui2_mean
SET_ENC_ACTS = {"tanh": 2, "softplus": 3}


def set_encode_route(N, widths, pool, act, needs_grad, double_backward, options=None) -> bool:
    """Does the stack ``phi`` with the max behind it run on ``set_encode_launch`` (mpg_set_encode_fwd)?  ``widths`` = [K_0, D_0, ..,
    D_{L-1}]; ``pool`` in 1 .. 3 (or a name of ``SET_ENC_POOLS``), ``act`` in 2, 3 (or a name of ``SET_ENC_ACTS``).  With the
    option on (``OPTIONS["set_encode"]``), when nothing in the call needs a gradient (``needs_grad``: grad mode is on and the input
    or a parameter of the stack requires grad -- the launch is forward only, the reference runs this encoder frozen), outside the
    double-backward route, and inside the kernel's limits: 1 <= N <= 128, 1 <= L <= 4, every width in 1 .. 256.  Host only."""
    opt = OPTIONS if options is None else options
    if not opt.get("set_encode") or needs_grad or double_backward:
        return False
    max_n, max_d, max_l = SET_ENC_MAX
    if SET_ENC_POOLS.get(pool, pool) not in (1, 2, 3) or SET_ENC_ACTS.get(act, act) not in (2, 3):
        return False
    return 1 <= int(N) <= max_n and 2 <= len(widths) <= max_l + 1 and all(1 <= int(w) <= max_d for w in widths)


def set_encode_launch(x, gammas, biases, lambdas, *, pool, act, pooled=None):
    """The launch: pooled [B, D_{L-1}] from ``x`` [B, N, K_0] (unit column stride, rows ``x.stride(1)`` apart, jets N rows apart),
    the layers' ``gammas`` [D_l, K_l], ``biases`` [D_l] (entries may be None) and, for pools 2 and 3, ``lambdas`` [D_l, K_l] -- the
    parameters themselves where they are contiguous.  ``pooled``: a caller-owned [B, >= D] row view to write into."""
    _chk(x, "x")
    B, N, K0 = x.shape
    if x.stride(2) != 1 or x.stride(1) < K0 or x.stride(0) != N * x.stride(1):
        x = x.contiguous()
    pool, act = SET_ENC_POOLS.get(pool, pool), SET_ENC_ACTS.get(act, act)
    L = len(gammas)
    if L > SET_ENC_MAX[2]:
        raise ValueError(f"set_encode: at most {SET_ENC_MAX[2]} layers, got {L}")
    if pooled is None:
        pooled = torch.empty((B, gammas[-1].shape[0]), device=x.device, dtype=torch.float32)
    e = _lib.MpgSetEncode()
    e.x, e.ldx, e.B, e.N, e.L, e.pool, e.act = _p(x), x.stride(1), B, N, L, pool, act
    keep = []      # (contiguous copies live until the launch is enqueued; the stream orders their release)
    for l in range(L):
        G = gammas[l]
        _chk(G, "Gamma")
        e.K[l], e.D[l] = G.shape[1], G.shape[0]
        ws = [G, biases[l], lambdas[l] if pool != 1 else None]
        ws = [None if w is None else (w if w.is_contiguous() else w.contiguous()) for w in ws]
        keep.append(ws)
        e.Gamma[l], e.bias[l], e.Lambda[l] = (None if w is None else w.data_ptr() for w in ws)
    e.pooled, e.ld_pooled = _p(pooled), pooled.stride(0)
    check(_lib.lib().mpg_set_encode_fwd(C.byref(e), _stream()), "mpg_set_encode_fwd")
    return pooled


# ---- LinearNet as one twice-differentiable op (the gradient penalty; OPTIONS["gp_chain"]) ----------------------------------------
# On rows X_0 = (A | A2), with K_l the dropout keep-and-scale of layer l and G_l = K_l lrelu'(Z_l) (lrelu' = 1 on a layer without
# activation), constant almost everywhere:
#   forward       Z_l = X_{l-1} W_l^T + b_l ,  X_l = K_l lrelu(Z_l) = G_l Z_l                          l = 1..L   (+ resid on X_L)
#   first order   dZ_L = G_L Y_bar ,  dZ_{l-1} = G_{l-1} (dZ_l W_l) ,  x_bar = dZ_1 W_1 ,  W_bar_l = dZ_l^T X_{l-1} ,  b_bar_l = colsum dZ_l
#   second order  (u on x_bar, Phi = <u, x_bar>)   T_0 = u ,  T_l = G_l (T_{l-1} W_l^T)
#                 dPhi/dY_bar = T_L ,  dPhi/dW_l = dZ_l^T T_{l-1} ,  dPhi/dX_0 = 0 ,  dPhi/db_l = 0
# All three passes are mpg_chain launches on bf16 hi/lo images (three terms: cotangents and tangents of any magnitude pass): the
# forward chain with per-layer outputs; the input-gradient chain with gateH = X_{l-1} and per-layer out = dZ_l; the tangent chain in
# the forward form with act = 0, no bias and gateH = X_l.  mpg_chain's gate on its INPUT is the dropout keep alone (in_thr): where the
# op's last layer has an activation (a net without final_linear, the leading ops of a net of more than three layers) dZ_L comes
# from one mpg_gate launch in front of the chain -- the one field the chain lacks (an input gateH).  All W_bar / dPhi/dW of an op
# come from one grouped split-K launch (``WgradBatch``).  The masks are regenerated from (tag, thr) in the gates, never stored;
# ``dropout_mask(rows, width, tag + 1 + l, thr)`` is layer l's (0-based; ``tag`` = the op's ``next_tag``).
CHAIN_OP_LAYERS = 3
LinearNetSettings = namedtuple("LinearNetSettings", "acts alpha p_drop training keeps param_grads", defaults=(0.2, 0.0, True, None, True))


class PackedLinearNet(_PackedSet):
    """The images one ``LinearNetFn`` call needs: W_l as the forward and tangent chains apply it and its transpose for the
    input-gradient chain, bf16 hi/lo, one ``mpg_pack_many`` launch."""

    def __init__(self, weights):
        spec = {}
        for l, W in enumerate(weights):
            n, k = W.shape
            spec[f"W{l}"] = (W, n, k, 0, 1.0, False, 0, 0)
            spec[f"W{l}T"] = (W, k, n, 1, 1.0, False, 0, 0)
        super().__init__(tuple(weights), spec)


def _chain_sizes_ok(widths) -> bool:
    # would mpg_chain take layers of these widths (K = widths[l], N = widths[l + 1])?  Sizes only: no pointer is dereferenced
    c = MpgChain()
    c.A, c.lda, c.K1, c.a_slabs = C.c_void_p(16), widths[0], widths[0], 1
    c.M, c.nlayers, c.alpha = 32, len(widths) - 1, 0.2
    for l in range(len(widths) - 1):
        c.L[l].K, c.L[l].N = widths[l], widths[l + 1]
    return chain_route(c) > 0


def gp_chain_pieces(nlayers: int):
    """The layer ranges [i0, i1) of the consecutive ops a net of ``nlayers`` layers runs as (``CHAIN_OP_LAYERS`` each at most)."""
    return [(i0, min(i0 + CHAIN_OP_LAYERS, nlayers)) for i0 in range(0, nlayers, CHAIN_OP_LAYERS)]


def gp_chain_route(widths, final_linear, batch_norm, spectral_norm, double_backward, options=None) -> bool:
    """Does a LinearNet call inside ``double_backward_route`` take ``LinearNetFn`` instead of the composites of
    ``LinearNet._forward_dd``?  Only with the option on (``OPTIONS["gp_chain"]``), for a plain net (no batch norm, no spectral norm)
    every piece of which ``mpg_chain_route`` accepts in the forward and in the input-gradient direction (``widths``: input width,
    then every layer's output width).  ``final_linear`` does not restrict anything: a last layer with an activation costs one
    ``mpg_gate`` launch.  Host only."""
    opt = OPTIONS if options is None else options
    if not (opt.get("gp_chain") and double_backward) or batch_norm or spectral_norm or len(widths) < 2 or min(widths) < 1:
        return False
    widths = [int(v) for v in widths]
    for i0, i1 in gp_chain_pieces(len(widths) - 1):
        w = widths[i0:i1 + 1]
        if not (_chain_sizes_ok(w) and _chain_sizes_ok(w[::-1])):
            return False
    return True


class _NetState:
    """What one ``LinearNetFn`` call keeps for its two derivatives beside its saved inputs."""
    __slots__ = ("cpu", "M", "K1", "L", "widths", "acts", "alpha", "thr", "dscale", "tag", "seed_t", "pk", "X", "G", "param_grads",
                 "has_bias", "has_resid")


def _net_gate(st, l, Y):
    # the ``gate`` entry of a chain layer that multiplies by G_l (0-based l), or None where G_l = 1.  ``st.X`` holds the outputs of
    # every layer but the last, whose output ``Y`` is the op's own (saved as an output, not on the state: no reference cycle)
    X = Y if l == st.L - 1 else st.X[l]
    return (X, st.acts[l], st.tag + 1 + l, st.thr, st.dscale) if (st.acts[l] or st.thr) else None


class LinearNetFn(torch.autograd.Function):
    """Up to three layers of a plain LinearNet on rows (A | A2) [M, K1 + K2], twice differentiable: see above.  ``resid`` [M, N_L] or
    None is added to the output (only behind a last layer without activation); ``settings``: a ``LinearNetSettings`` -- ``acts`` one
    flag per layer, ``keeps`` the keep-and-scale masks of a CPU call (None: no dropout), ``param_grads`` False: a first derivative
    taken with ``create_graph=True`` forms no parameter gradients (the penalty differentiates with respect to the input alone).
    ``params``: W_1, b_1, ..., W_L, b_L (a bias may be None).  CPU tensors take the same formulas in plain torch, in their dtype."""

    @staticmethod
    def forward(ctx, A, A2, resid, settings, *params):
        s = settings
        Ws, bs = params[0::2], params[1::2]
        L = len(Ws)
        if not (1 <= L <= CHAIN_OP_LAYERS and len(s.acts) == L and len(bs) == L):
            raise ValueError(f"LinearNetFn: 1..{CHAIN_OP_LAYERS} layers with a flag and a bias slot each, got {L}")
        if resid is not None and s.acts[-1]:
            raise NotImplementedError("LinearNetFn: a residual needs a last layer without activation")
        st = _NetState()
        st.cpu, st.M, st.K1, st.L = not A.is_cuda, A.shape[0], A.shape[1], L
        st.widths = [A.shape[1] + (0 if A2 is None else A2.shape[1])] + [W.shape[0] for W in Ws]
        st.acts, st.alpha, st.param_grads = tuple(bool(a) for a in s.acts), float(s.alpha), bool(s.param_grads)
        st.has_bias, st.has_resid = tuple(b is not None for b in bs), resid is not None
        ctx.st = st
        if st.cpu:
            h = A if A2 is None else torch.cat((A, A2), 1)
            st.X, st.G = [], []
            for l in range(L):
                Z = h @ Ws[l].t()
                if bs[l] is not None:
                    Z = Z + bs[l]
                g = torch.where(Z > 0, torch.ones_like(Z), torch.full_like(Z, st.alpha)) if st.acts[l] else torch.ones_like(Z)
                if s.keeps is not None and s.keeps[l] is not None:
                    g = g * s.keeps[l]
                h = g * Z
                st.G.append(g)
                if l < L - 1:
                    st.X.append(h)
            out = h if resid is None else h + resid
            ctx.save_for_backward(A, A2, out, *params)
            return out
        _chk(A, "A")
        dev, M = A.device, st.M
        st.thr, st.dscale = drop_params(s.p_drop) if s.training else (0, 1.0)
        st.seed_t, st.tag = seed_tensor(dev), next_tag(dev, "linear_net", st.thr)
        st.pk = PackedLinearNet(Ws).ensure()
        A, A2 = _unit_cols(A), None if A2 is None else _unit_cols(A2)
        r2 = None if resid is None else _unit_cols(resid)
        X = [torch.empty((M, n), device=dev, dtype=torch.float32) for n in st.widths[1:]]
        layers = [dict(img=st.pk.ptr(f"W{l}"), K=st.widths[l], N=st.widths[l + 1], bias=bs[l], act=st.acts[l],
                       drop=(st.tag + 1 + l, st.thr, st.dscale), out=X[l], resid=r2 if l == L - 1 else None) for l in range(L)]
        run_chain(chain_struct(M, layers, A=A, lda=A.stride(0), K1=st.K1, A2=A2, lda2=0 if A2 is None else A2.stride(0),
                               alpha=st.alpha, seed_t=st.seed_t, f16=False))
        st.X = X[:-1]
        ctx.save_for_backward(A, A2, X[-1], *params)
        return X[-1]

    @staticmethod
    def backward(ctx, ybar):
        A, A2, Y, *params = ctx.saved_tensors
        need, st = ctx.needs_input_grad, ctx.st
        again = torch.is_grad_enabled()     # (create_graph=True: this derivative will be differentiated itself)
        flags = (need[0] or (A2 is not None and need[1]), any(need[4:]) and (st.param_grads or not again), again)
        out = LinearNetVJPFn.apply(ybar, A, A2, Y.detach(), st, flags, *params)
        return (out[0] if need[0] else None, out[1] if need[1] else None, ybar if (st.has_resid and need[2]) else None, None, *out[2:])


class LinearNetVJPFn(torch.autograd.Function):
    """The first derivative of ``LinearNetFn`` as a function of (Y_bar, A, A2, parameters): (A_bar, A2_bar, W_bar_1, b_bar_1, ...).
    Its own backward takes cotangents on A_bar and A2_bar (an absent one is zero) -- one on a parameter gradient raises -- and is
    once differentiable: a third derivative declines loudly."""

    @staticmethod
    def forward(ctx, ybar, A, A2, Y, st, flags, *params):
        need_x, need_w, again = flags
        Ws = params[0::2]
        L, K1 = st.L, st.K1
        ctx.st, ctx.flags = st, flags
        ctx.set_materialize_grads(False)
        pg = [None] * (2 * L)
        ctx.save_for_backward(Y, *Ws)
        if st.cpu:
            dZ, d = [None] * L, st.G[L - 1] * ybar
            for l in range(L - 1, -1, -1):
                dZ[l] = d
                if l > 0:
                    d = st.G[l - 1] * (d @ Ws[l])
            ctx.dz = dZ
            xbar = dZ[0] @ Ws[0] if need_x else None
            if need_w:
                X0 = A if A2 is None else torch.cat((A, A2), 1)
                for l in range(L):
                    pg[2 * l] = dZ[l].t() @ (X0 if l == 0 else st.X[l - 1])
                    pg[2 * l + 1] = dZ[l].sum(0) if st.has_bias[l] else None
            return (None if xbar is None else xbar[:, :K1], None if (xbar is None or A2 is None) else xbar[:, K1:], *pg)
        dev, M, w = ybar.device, st.M, st.widths
        yb = ybar.reshape(M, w[L]).float().contiguous()
        A, A2 = _unit_cols(A), None if A2 is None else _unit_cols(A2)
        keep_dz = need_w or again
        nchain = L - 1 + int(need_x)     # layers of the input-gradient chain
        in_gate = in_out = None
        if st.acts[L - 1] or (st.thr and nchain == 0):
            dZL = gate(yb, Y if st.acts[L - 1] else None, gate_act=st.acts[L - 1], alpha=st.alpha, seed_t=st.seed_t, tag=st.tag + L,
                       thr=st.thr, scale=st.dscale)
        elif st.thr:
            dZL = torch.empty_like(yb)
            in_gate, in_out = (st.tag + L, st.thr, st.dscale), dZL
        else:
            dZL = yb
        dZ = [None] * L
        dZ[L - 1] = dZL
        xbar = torch.empty((M, w[0]), device=dev, dtype=torch.float32) if need_x else None
        if nchain:
            layers = []
            for l in range(L - 1, 0, -1):
                if keep_dz:   # (dZ_l leaves the chip only for a weight gradient or the second derivative)
                    dZ[l - 1] = torch.empty((M, w[l]), device=dev, dtype=torch.float32)
                layers.append(dict(img=st.pk.ptr(f"W{l}T"), K=w[l + 1], N=w[l], gate=_net_gate(st, l - 1, Y), out=dZ[l - 1]))
            if need_x:
                layers.append(dict(img=st.pk.ptr("W0T"), K=w[1], N=w[0], out=xbar))
            run_chain(chain_struct(M, layers, A=yb if in_gate is not None else dZL, lda=w[L], K1=w[L], in_gate=in_gate, in_out=in_out,
                                   alpha=st.alpha, seed_t=st.seed_t, f16=False))
        ctx.dz = dZ if again else None
        if need_w:
            wb = WgradBatch()
            for l in range(L):
                W = Ws[l]
                pg[2 * l] = torch.empty_like(W)
                pg[2 * l + 1] = torch.empty((W.shape[0],), device=dev, dtype=torch.float32) if st.has_bias[l] else None
                if l == 0:
                    wb.add(dZ[0], A, out=pg[0], out_col0=0, bias_out=pg[1])
                    if A2 is not None:
                        wb.add(dZ[0], A2, out=pg[0], out_col0=K1)
                else:
                    wb.add(dZ[l], st.X[l - 1], out=pg[2 * l], bias_out=pg[2 * l + 1])
            wb.flush()
        return (None if xbar is None else xbar[:, :K1], None if (xbar is None or A2 is None) else xbar[:, K1:], *pg)

    @staticmethod
    @once_differentiable
    def backward(ctx, uA, uA2, *gparams):
        if any(g is not None for g in gparams):
            raise RuntimeError("LinearNetVJPFn: a cotangent arrived on a parameter-gradient output; the second-order rule covers the "
                               "input gradient only")
        st = ctx.st
        if ctx.dz is None:
            raise RuntimeError("LinearNetVJPFn: the first derivative was taken without create_graph=True; there is nothing to differentiate again")
        L, K1, w, dZ = st.L, st.K1, st.widths, ctx.dz
        need_w = [ctx.needs_input_grad[6 + 2 * l] for l in range(L)]
        gW = [None] * L
        two = w[0] > K1
        Y, *Ws = ctx.saved_tensors
        if st.cpu:
            ref = dZ[0]
            zero = lambda k: torch.zeros((st.M, k), dtype=ref.dtype)
            T = torch.cat((zero(K1) if uA is None else uA, *(((zero(w[0] - K1) if uA2 is None else uA2),) if two else ())), 1)
            for l in range(L):
                if need_w[l]:
                    gW[l] = dZ[l].t() @ T
                T = st.G[l] * (T @ Ws[l].t())
            return (T, None, None, None, None, None, *(q for g in gW for q in (g, None)))
        dev, M = dZ[-1].device, st.M
        zero = lambda k: torch.zeros((M, k), device=dev, dtype=torch.float32)
        uA = zero(K1) if uA is None else _unit_cols(uA.reshape(M, K1).float())
        uA2 = None if not two else (zero(w[0] - K1) if uA2 is None else _unit_cols(uA2.reshape(M, w[0] - K1).float()))
        T = [torch.empty((M, w[l + 1]), device=dev, dtype=torch.float32) if (l == L - 1 or need_w[l + 1]) else None for l in range(L)]
        layers = [dict(img=st.pk.ptr(f"W{l}"), K=w[l], N=w[l + 1], act=False, gate=_net_gate(st, l, Y), out=T[l]) for l in range(L)]
        run_chain(chain_struct(M, layers, A=uA, lda=uA.stride(0), K1=K1, A2=uA2, lda2=0 if uA2 is None else uA2.stride(0),
                               alpha=st.alpha, seed_t=st.seed_t, f16=False))
        if any(need_w):
            wb = WgradBatch()
            for l in range(L):
                if not need_w[l]:
                    continue
                gW[l] = torch.empty((w[l + 1], w[l]), device=dev, dtype=torch.float32)
                if l == 0:
                    wb.add(dZ[0], uA, out=gW[0], out_col0=0)
                    if two:
                        wb.add(dZ[0], uA2, out=gW[0], out_col0=K1)
                else:
                    wb.add(dZ[l], T[l - 1], out=gW[l])
            wb.flush()
        return (T[L - 1], None, None, None, None, None, *(q for g in gW for q in (g, None)))


def linear_net_dd(A, A2, weights, biases, *, final_linear, alpha, p_drop, training, resid=None, keeps=None, param_grads=False):
    """A plain LinearNet on rows (A | A2) as consecutive ``LinearNetFn`` ops of up to ``CHAIN_OP_LAYERS`` layers each.  ``resid`` goes
    into the last op's launch when the last layer has no activation, else it is added behind it."""
    L = len(weights)
    acts = [not (final_linear and l == L - 1) for l in range(L)]
    fuse = resid is not None and not acts[-1]
    h, h2 = A, A2
    for i0, i1 in gp_chain_pieces(L):
        s = LinearNetSettings(tuple(acts[i0:i1]), alpha, p_drop, training, None if keeps is None else keeps[i0:i1], param_grads)
        prm = [q for W, b in zip(weights[i0:i1], biases[i0:i1]) for q in (W, b)]
        h, h2 = LinearNetFn.apply(h, h2, resid if (fuse and i1 == L) else None, s, *prm), None
    return h if (resid is None or fuse) else h + resid


class FusedDropoutFn(torch.autograd.Function):
    """Stand-alone inverted dropout on the counter-based mask stream (MAB.dropout, gapt/model.py:132,137)."""

    @staticmethod
    def forward(ctx, x, p_drop, training):
        thr, scale = drop_params(p_drop) if training else (0, 1.0)
        if not thr:
            ctx.cfg = None
            return x
        _chk(x, "x")
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        tag = next_tag(x.device, "dropout", thr) + TAG_GENERIC
        ctx.cfg = (tag, thr, scale, x.shape)
        return gate(x2, None, gate_act=False, alpha=0.0, seed_t=seed_tensor(x.device), tag=tag, thr=thr,
                    scale=scale).reshape(x.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if ctx.cfg is None:
            return g, None, None
        tag, thr, scale, shp = ctx.cfg
        g2 = g.reshape(-1, shp[-1]).contiguous()
        return gate(g2, None, gate_act=False, alpha=0.0, seed_t=seed_tensor(g.device), tag=tag, thr=thr,
                    scale=scale).reshape(shp), None, None


class KeyedDropoutFn(torch.autograd.Function):
    """``FusedDropoutFn``'s mask stream as an op that can be differentiated to any order: dropout is linear in x, so its backward is
    the op itself on the cotangent, with the same site tag (the mask is regenerated, never stored)."""

    @staticmethod
    def forward(ctx, x, tag, thr, scale):
        _chk(x, "x")
        ctx.cfg = (tag, thr, scale)
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        return gate(x2, None, gate_act=False, alpha=0.0, seed_t=seed_tensor(x.device), tag=tag, thr=thr, scale=scale).reshape(x.shape)

    @staticmethod
    def backward(ctx, g):
        return KeyedDropoutFn.apply(g, *ctx.cfg), None, None, None


def keyed_dropout(x, p_drop, training):
    """Stand-alone inverted dropout inside ``double_backward_route`` drawn from the device seed and ``next_tag`` (``OPTIONS["gp_chain"]``:
    MAB's two dropouts of the gradient penalty), in place of ATen's draw from torch's generator."""
    thr, scale = drop_params(p_drop) if training else (0, 1.0)
    if not thr:
        return x
    return KeyedDropoutFn.apply(x, next_tag(x.device, "dropout", thr) + TAG_GENERIC, thr, scale)


def _attn_struct(q, k, v, ignore, o, P, B, L, S, H, d):
    a = _lib.MpgAttn()
    a.q, a.k, a.v = _p(q), _p(k), _p(v)
    a.ldq, a.ldk, a.ldv = q.stride(0), k.stride(0), v.stride(0)
    a.ignore = _p(ignore)
    a.o, a.ldo, a.P = _p(o), o.stride(0), _p(P)
    a.B, a.L, a.S, a.H, a.d = B, L, S, H, d
    return a


class FusedPackedAttnFn(torch.autograd.Function):
    """FusedAttnFn on PACKED projections, as MAB produces them: self-attention takes qkv [B*L, 3E] (kv = None),
    cross-attention q [B*L, E] and kv [B*S, 2E].  The backward writes dq / dk / dv straight into one gradient
    tensor per packed input -- slicing q, k, v out in autograd instead costs a zero-fill, a copy and an add per slice."""

    @staticmethod
    def forward(ctx, qx, kv, ignore, B, L, S, H):
        _chk(qx, "qkv")
        self_attn = kv is None
        E = qx.shape[1] // 3 if self_attn else qx.shape[1]
        d = E // H
        q = qx[:, :E]
        k, v = (qx[:, E:2 * E], qx[:, 2 * E:]) if self_attn else (kv[:, :E], kv[:, E:])
        o = torch.empty((B * L, E), device=qx.device, dtype=torch.float32)
        P = torch.empty((B, H, L, S), device=qx.device, dtype=torch.float32)
        a = _attn_struct(q, k, v, ignore, o, P, B, L, S, H, d)
        check(_lib.lib().mpg_attn_fwd(C.byref(a), _stream()), "mpg_attn_fwd")
        ctx.save_for_backward(qx, kv, P)
        ctx.ignore = ignore
        ctx.dims = (B, L, S, H, d, E, self_attn)
        return o

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        qx, kv, P = ctx.saved_tensors
        B, L, S, H, d, E, self_attn = ctx.dims
        go = go.contiguous()
        dqx = torch.empty_like(qx)
        dkv = None if self_attn else torch.empty_like(kv)
        q = qx[:, :E]
        k, v = (qx[:, E:2 * E], qx[:, 2 * E:]) if self_attn else (kv[:, :E], kv[:, E:])
        dq = dqx[:, :E]
        dk, dv = (dqx[:, E:2 * E], dqx[:, 2 * E:]) if self_attn else (dkv[:, :E], dkv[:, E:])
        a = _attn_struct(q, k, v, ctx.ignore, go, P, B, L, S, H, d)
        a.d_o = _p(go)
        a.dq, a.dk, a.dv = C.c_void_p(dq.data_ptr()), C.c_void_p(dk.data_ptr()), C.c_void_p(dv.data_ptr())
        a.lddq, a.lddk, a.lddv = dq.stride(0), dk.stride(0), dv.stride(0)
        check(_lib.lib().mpg_attn_bwd(C.byref(a), _stream()), "mpg_attn_bwd")
        return dqx, dkv, None, None, None, None, None


class FusedAttnFn(torch.autograd.Function):
    """softmax(q k^T / sqrt(d) + key mask) v per (jet, head): q [B*L, E], k, v [B*S, E] (row-strided
    views are fine), ignore [B*S] floats (1 = padded key) or None."""

    @staticmethod
    def forward(ctx, q, k, v, ignore, B, L, S, H):
        _chk(q, "q")
        E = q.shape[1]
        d = E // H
        o = torch.empty((B * L, E), device=q.device, dtype=torch.float32)
        P = torch.empty((B, H, L, S), device=q.device, dtype=torch.float32)
        a = _attn_struct(q, k, v, ignore, o, P, B, L, S, H, d)
        check(_lib.lib().mpg_attn_fwd(C.byref(a), _stream()), "mpg_attn_fwd")
        ctx.save_for_backward(q, k, v, P)
        ctx.ignore = ignore
        ctx.dims = (B, L, S, H, d)
        return o

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        q, k, v, P = ctx.saved_tensors
        B, L, S, H, d = ctx.dims
        go = go.contiguous()
        dq = torch.empty((B * L, H * d), device=q.device, dtype=torch.float32)
        dk = torch.empty((B * S, H * d), device=q.device, dtype=torch.float32)
        dv = torch.empty((B * S, H * d), device=q.device, dtype=torch.float32)
        a = _attn_struct(q, k, v, ctx.ignore, go, P, B, L, S, H, d)
        a.d_o = _p(go)
        a.dq, a.dk, a.dv = _p(dq), _p(dk), _p(dv)
        a.lddq, a.lddk, a.lddv = H * d, H * d, H * d
        check(_lib.lib().mpg_attn_bwd(C.byref(a), _stream()), "mpg_attn_bwd")
        return dq, dk, dv, None, None, None, None, None


# ---- the attention core, twice differentiable (the gradient penalty through GAPT's MAB)
#   AttnCoreFn      forward: ``mpg_attn_fwd``; backward: ``AttnCoreVJPFn``.
#   AttnCoreVJPFn   forward: the first derivative (dq, dk, dv) as a function of (d_o, q, k, v) on ``mpg_attn_bwd``; backward (once
#                   differentiable): the gradients of Phi = <uq, dq> + <uk, dk> + <uv, dv> on ``mpg_attn_dd``.
# CPU tensors take the same formulas in plain torch, in the tensors' dtype.
ATTN_DD_MAX_TOKENS = 160     # mpg_attn_dd: queries / keys of a (jet, head) pair
ATTN_DD_HEAD_DIMS = (8, 16, 32)


def gp_attn_route(E, H, L, S, *, double_backward, options=None) -> bool:
    """Does a MAB call inside ``double_backward_route`` take ``AttnCoreFn`` for softmax(q k^T / sqrt(d)) v instead of the broadcast
    products of ``MAB._forward_dd``?  Only with the option on (``OPTIONS["gp_attn"]``) and for the shapes ``mpg_attn_dd`` covers: heads
    of 8, 16 or 32 features, 1 <= L, S <= ``ATTN_DD_MAX_TOKENS``.  Host only: sizes and the switch decide."""
    opt = OPTIONS if options is None else options
    if not (opt.get("gp_attn") and double_backward):
        return False
    return H > 0 and E % H == 0 and E // H in ATTN_DD_HEAD_DIMS and 1 <= L <= ATTN_DD_MAX_TOKENS and 1 <= S <= ATTN_DD_MAX_TOKENS


def _attn_heads(t, B, T, H, d):
    return t.reshape(B, T, H, d).permute(0, 2, 1, 3)          # [rows, E] -> [B, H, T, d]


def _attn_rows(t, B, T, H, d):
    return t.permute(0, 2, 1, 3).reshape(B * T, H * d)


def _attn_probs_cpu(q, k, ignore, dims):
    B, L, S, H, d = dims
    s = _attn_heads(q, B, L, H, d) @ _attn_heads(k, B, S, H, d).transpose(2, 3) * (1.0 / d ** 0.5)
    if ignore is None:
        return torch.softmax(s, -1)
    ig = ignore.reshape(B, 1, 1, S) != 0
    dead = ig.all(dim=-1, keepdim=True)
    return torch.softmax(s.masked_fill(ig & ~dead, float("-inf")), -1) * (~dead).to(s.dtype)


def _attn_launch_rows(t, E):
    # what the kernels take as a [rows, E] operand: unit column stride, a row stride of at least the width
    return t if (t.stride(1) == 1 and t.stride(0) >= E) else t.contiguous()


class AttnCoreFn(torch.autograd.Function):
    """softmax(q k^T / sqrt(d) + key mask) v per (jet, head) as ``FusedAttnFn`` computes it -- q [B*L, E], k, v [B*S, E] (row-strided
    views are fine), ignore [B*S] floats (1 = padded key) or None -- and twice differentiable: its backward is ``AttnCoreVJPFn``."""

    @staticmethod
    def forward(ctx, q, k, v, ignore, B, L, S, H):
        E = q.shape[1]
        d = E // H
        ctx.dims, ctx.ignore = (B, L, S, H, d), ignore
        if not q.is_cuda:
            P = _attn_probs_cpu(q, k, ignore, ctx.dims)
            ctx.save_for_backward(q, k, v, P)
            return _attn_rows(P @ _attn_heads(v, B, S, H, d), B, L, H, d)
        _chk(q, "q")
        ql, kl, vl = (_attn_launch_rows(t, E) for t in (q, k, v))
        o = torch.empty((B * L, E), device=q.device, dtype=torch.float32)
        P = torch.empty((B, H, L, S), device=q.device, dtype=torch.float32)   # (layout private to the kernels)
        a = _attn_struct(ql, kl, vl, ignore, o, P, B, L, S, H, d)
        check(_lib.lib().mpg_attn_fwd(C.byref(a), _stream()), "mpg_attn_fwd")
        ctx.save_for_backward(q, k, v, P)     # (the inputs themselves: the second derivative flows back through them)
        return o

    @staticmethod
    def backward(ctx, go):
        q, k, v, P = ctx.saved_tensors
        return (*AttnCoreVJPFn.apply(go, q, k, v, P, ctx.ignore, ctx.dims), None, None, None, None, None)


class AttnCoreVJPFn(torch.autograd.Function):
    """The first derivative of ``AttnCoreFn`` as a function of (d_o, q, k, v): (dq, dk, dv).  Its own backward takes cotangents uq,
    uk, uv on them -- an absent one is zero -- and is once differentiable: a third derivative declines loudly."""

    @staticmethod
    def forward(ctx, go, q, k, v, P, ignore, dims):
        B, L, S, H, d = dims
        ctx.dims, ctx.ignore = dims, ignore
        ctx.set_materialize_grads(False)
        if not q.is_cuda:
            ctx.save_for_backward(go, q, k, v, P)
            c = 1.0 / d ** 0.5
            G, qh, kh, vh = _attn_heads(go, B, L, H, d), _attn_heads(q, B, L, H, d), _attn_heads(k, B, S, H, d), _attn_heads(v, B, S, H, d)
            A = G @ vh.transpose(2, 3)
            dS = P * (A - (P * A).sum(-1, keepdim=True))
            return (_attn_rows(c * (dS @ kh), B, L, H, d), _attn_rows(c * (dS.transpose(2, 3) @ qh), B, S, H, d),
                    _attn_rows(P.transpose(2, 3) @ G, B, S, H, d))
        E = H * d
        go, q, k, v = (_attn_launch_rows(t.float(), E) for t in (go, q, k, v))
        dq = torch.empty((B * L, E), device=q.device, dtype=torch.float32)
        dk = torch.empty((B * S, E), device=q.device, dtype=torch.float32)
        dv = torch.empty((B * S, E), device=q.device, dtype=torch.float32)
        a = _attn_struct(q, k, v, ignore, go, P, B, L, S, H, d)
        a.d_o = _p(go)
        a.dq, a.dk, a.dv = _p(dq), _p(dk), _p(dv)
        a.lddq, a.lddk, a.lddv = E, E, E
        check(_lib.lib().mpg_attn_bwd(C.byref(a), _stream()), "mpg_attn_bwd")
        ctx.save_for_backward(go, q, k, v, P)
        return dq, dk, dv

    @staticmethod
    @once_differentiable
    def backward(ctx, uq, uk, uv):
        go, q, k, v, P = ctx.saved_tensors
        B, L, S, H, d = ctx.dims
        n_go, n_q, n_k, n_v = ctx.needs_input_grad[:4]
        tail = (None, None, None)
        if uq is None and uk is None and uv is None:
            return (None, None, None, None, *tail)
        if not q.is_cuda:
            c = 1.0 / d ** 0.5
            hl, hs = (lambda t: _attn_heads(t, B, L, H, d)), (lambda t: _attn_heads(t, B, S, H, d))
            G, qh, kh, vh = hl(go), hl(q), hs(k), hs(v)
            rowsum = lambda X: (P * X).sum(-1, keepdim=True)
            A = G @ vh.transpose(2, 3)
            Aa = A - rowsum(A)
            dS = P * Aa
            Sd = torch.zeros_like(P)
            if uq is not None:
                Sd = Sd + c * (hl(uq) @ kh.transpose(2, 3))
            if uk is not None:
                Sd = Sd + c * (qh @ hs(uk).transpose(2, 3))
            r = rowsum(Sd)
            Pd = P * (Sd - r)
            M = Sd * Aa - r * A
            if uv is not None:
                M = M + G @ hs(uv).transpose(2, 3)
            D2 = P * (M - rowsum(M))
            g_q = c * (D2 @ kh)
            if uk is not None:
                g_q = g_q + c * (dS @ hs(uk))
            g_k = c * (D2.transpose(2, 3) @ qh)
            if uq is not None:
                g_k = g_k + c * (dS.transpose(2, 3) @ hl(uq))
            g_v = Pd.transpose(2, 3) @ G
            g_go = Pd @ vh
            if uv is not None:
                g_go = g_go + P @ hs(uv)
            return (_attn_rows(g_go, B, L, H, d), _attn_rows(g_q, B, L, H, d), _attn_rows(g_k, B, S, H, d),
                    _attn_rows(g_v, B, S, H, d), *tail)
        E, dev = H * d, q.device
        e = _lib.MpgAttnDD()
        e.q, e.k, e.v, e.d_o = _p(q), _p(k), _p(v), _p(go)
        e.ldq, e.ldk, e.ldv, e.ldo = q.stride(0), k.stride(0), v.stride(0), go.stride(0)
        keep = []
        for name, u, rows in (("uq", uq, B * L), ("uk", uk, B * S), ("uv", uv, B * S)):
            if u is not None:
                u = _attn_launch_rows(u.float(), E)
                if tuple(u.shape) != (rows, E):
                    raise ValueError(f"AttnCoreVJPFn: cotangent {name} has shape {tuple(u.shape)}, expected {(rows, E)}")
                keep.append(u)
                setattr(e, name, _p(u)); setattr(e, "ld" + name, u.stride(0))
        e.ignore, e.P = _p(ctx.ignore), _p(P)
        out = []
        for name, need, rows in (("gdo", n_go, B * L), ("gq", n_q, B * L), ("gk", n_k, B * S), ("gv", n_v, B * S)):
            g = torch.empty((rows, E), device=dev, dtype=torch.float32) if need else None
            setattr(e, name, _p(g)); setattr(e, "ld" + name, E)
            out.append(g)
        e.B, e.L, e.S, e.H, e.d = B, L, S, H, d
        check(_lib.lib().mpg_attn_dd(C.byref(e), _stream()), "mpg_attn_dd")
        return (*out, *tail)


# ------------------------------------------------------------------------------------- one launch per MAB
class PackedMAB(_PackedSet):
    """Weight images of one MAB for ``mpg_mab_fwd`` / ``mpg_mab_bwd``: fp16 images of the three weights for the forward
    products, bf16 images of their transposes for the gradient products."""

    def __init__(self, Win, Wo, Wf):
        E = Wo.shape[0]
        super().__init__((Win, Wo, Wf), {
            "Win": (Win, 3 * E, E, 0, SC_WN, True, 0, 0), "Wo": (Wo, E, E, 0, SC_WN, True, 0, 0), "Wf": (Wf, E, E, 0, SC_WN, True, 0, 0),
            "WinT": (Win, E, 3 * E, 1, 1.0, False, 0, 0), "WoT": (Wo, E, E, 1, 1.0, False, 0, 0), "WfT": (Wf, E, E, 1, 1.0, False, 0, 0),
        })


def mab_fusable(E: int, H: int, L: int, S: int) -> bool:
    """Shapes ``mpg_mab_fwd`` / ``mpg_mab_bwd`` take: sets of at most 160 tokens (up to 32: a wave or two per jet; beyond: a
    workgroup per jet, a wave per tile of 32 tokens), E = 32 or 64, heads of 16 features."""
    return E in (32, 64) and H * 16 == E and 1 <= L <= MAB_MAX_TOKENS and 1 <= S <= MAB_MAX_TOKENS


MAB_MAX_TOKENS = 160
MAB_CHAIN_TOKENS = 32      # (``mpg_mab_chain_fwd`` keeps a jet's rows in one wave's registers)

# The six parameters of a block, as they travel together: in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias, ff weight, ff bias
MABParams = namedtuple("MABParams", "Win bin Wo bo Wf bf")
# The non-tensor state of one block invocation (``ctx.cfg``); p_mab / p_ff are the rates in force (0 outside training)
MABCfg = namedtuple("MABCfg", "B L S E H alpha ff_act tag p_mab p_ff")
# What a block's forward keeps for its backward, in ``save_for_backward`` order: the query rows, the key/value rows (None: self-attention),
# the key mask or None, o (attention output), z (input of the feed-forward layer) and -- None without LayerNorm -- za (input of norm1)
# and the norms' parameters
MABSaved = namedtuple("MABSaved", "x2 y2 ignore o z za n1w n1b n2w n2b", defaults=(None,) * 5)


def _groups(seq, n):
    return [tuple(seq[i:i + n]) for i in range(0, len(seq), n)]


def mab_saved(node):
    """The saved tensors of a ``FusedMABFn`` backward node (the ``grad_fn`` behind a one-launch block's output), by name."""
    return MABSaved(*node.saved_tensors)


def _mab_cfg(dev, B, L, S, E, H, alpha, ff_act, p_mab, p_ff, training):
    """The ``MABCfg`` of a fresh invocation: it draws the block's dropout tag."""
    p_mab, p_ff = (p_mab, p_ff) if training else (0.0, 0.0)
    tag = next_tag(dev, "mab", max(drop_params(p_mab)[0], drop_params(p_ff)[0]))
    return MABCfg(B, L, S, E, H, alpha, ff_act, tag, p_mab, p_ff)


def _mab_struct(cfg, x2, y2, ignore, pk, prm, ln=None):
    """``MpgMab`` with everything the forward and the backward share.  ``ln``: (norm1.weight, norm1.bias, norm2.weight, norm2.bias,
    eps) of a block with ``layer_norm=True``."""
    m = _lib.MpgMab()
    m.x, m.ldx = _p(x2), x2.stride(0)
    m.y, m.ldy = (_p(x2), x2.stride(0)) if y2 is None else (_p(y2), y2.stride(0))
    m.ignore = _p(ignore)
    m.Win, m.bin, m.Wo, m.bo, m.Wf, m.bf = pk.ptr("Win"), _p(prm.bin), pk.ptr("Wo"), _p(prm.bo), pk.ptr("Wf"), _p(prm.bf)
    m.WinT, m.WoT, m.WfT = pk.ptr("WinT"), pk.ptr("WoT"), pk.ptr("WfT")
    m.B, m.L, m.S, m.E, m.H = cfg.B, cfg.L, cfg.S, cfg.E, cfg.H
    m.alpha, m.ff_act = cfg.alpha, int(cfg.ff_act)
    m.seed, m.tag = _p(seed_tensor(x2.device)), cfg.tag
    (m.thr_mab, m.sc_mab), (m.thr_ff, m.sc_ff) = drop_params(cfg.p_mab), drop_params(cfg.p_ff)
    m.wscale, m.ascale = SC_WN, SC_ACT
    if ln is not None:
        w1, b1, w2, b2, eps = ln
        m.ln1_w, m.ln1_b, m.ln2_w, m.ln2_b, m.ln_eps = _p(w1), _p(b1), _p(w2), _p(b2), float(eps)
    return m


def mab_forward(cfg, x2, y2, ignore, pk, prm, *, save=False, ln=None):
    """``mpg_mab_fwd``: x2 [B*L, E] queries, y2 [B*S, E] keys/values or None (self-attention), ignore [B*S] floats or
    None.  Returns (out [B*L, E], MABSaved); o, z and -- with ``ln`` -- za exist only with ``save`` (what the backward needs)."""
    _chk(x2, "x")
    out = torch.empty((cfg.B * cfg.L, cfg.E), device=x2.device, dtype=torch.float32)
    o = torch.empty_like(out) if save else None
    z = torch.empty_like(out) if save else None
    za = torch.empty_like(out) if (save and ln is not None) else None
    m = _mab_struct(cfg, x2, y2, ignore, pk, prm, ln)
    m.out, m.ldo, m.save_o, m.save_z, m.save_za = _p(out), out.stride(0), _p(o), _p(z), _p(za)
    check(_lib.lib().mpg_mab_fwd(C.byref(m), _stream()), "mpg_mab_fwd")
    return out, MABSaved(x2, y2, ignore, o, z, za, *(ln[:4] if ln is not None else ()))


def _mab_rows(x, y):
    """The rows the kernels take of x [B, L, E] and y [B, S, E] or None: (x2, y2, B, L, S, shared).  ``shared``: x is ONE query
    row for all B > 1 jets of y (PMA's learned seed, gapt/model.py:170-174: ``S.repeat(B, 1, 1)``) -- read with row stride 0
    instead of being copied B times."""
    B, L, E = x.shape
    shared = B == 1 and L == 1 and y is not None and y.shape[0] > 1
    if shared:
        B = y.shape[0]
    S = L if y is None else y.shape[1]
    x2 = x.reshape(1, E).contiguous().expand(B, E) if shared else x.reshape(B * L, E).contiguous()
    y2 = None if y is None else y.reshape(B * S, E).contiguous()
    return x2, y2, B, L, S, shared


def _mab_run(x, y, ignore, pk, prm, ln, H, alpha, ff_act, p_mab, p_ff, training, save):
    """One block on x [B, L, E] / y [B, S, E] or None: (out [B, L, E], MABSaved, MABCfg, shared)."""
    x2, y2, B, L, S, shared = _mab_rows(x, y)
    cfg = _mab_cfg(x.device, B, L, S, x.shape[2], H, alpha, ff_act, p_mab, p_ff, training)
    out, saved = mab_forward(cfg, x2, y2, ignore, pk, prm, save=save, ln=ln)
    return out.reshape(B, L, cfg.E), saved, cfg, shared


def mab_block(x, y, ignore, pk, prm, ln, H, alpha, ff_act, p_mab, p_ff, training):
    """MAB.forward (gapt/model.py:124-139) as one launch: x [B, L, E] queries -- or the [1, 1, E] row all jets share, see
    ``_mab_rows`` --, y [B, S, E] keys/values or None for self-attention, ``prm`` the block's ``MABParams``, ``ln`` as in
    ``_mab_struct``.  With grad enabled through ``FusedMABFn``; without, nothing is kept (no o, z or za)."""
    if not torch.is_grad_enabled():
        return _mab_run(x, y, ignore, pk, prm, ln, H, alpha, ff_act, p_mab, p_ff, training, False)[0]
    if ln is not None and x.shape[0] == 1 and y is not None and y.shape[0] > 1:
        # the shared row of a layer_norm=True block is copied per jet: autograd sums its gradient over the jets
        # (without LayerNorm the backward of FusedMABFn does, from the stride-0 row)
        x = x.expand(y.shape[0], -1, -1)
    return FusedMABFn.apply(x, y, ignore, *prm, *(ln if ln is not None else (None,) * 5), H, alpha, ff_act, p_mab, p_ff, training, pk)


def _colsum_grad(st, prm, need, rows):
    """The gradient of ONE vector parameter that is the column sums of ``rows`` -- a LayerNorm's weight or bias from the rows the
    block's backward left, the seed row all jets share from dx: a bias-sum job of the grouped launch inside a TrainStep
    backward (then None), else summed here.  Each such parameter decides for itself."""
    pg = ParamGrads(st, (prm,), (need,))
    pg.colsum(0, rows)
    return pg.slots()[0]


def _mab_backward_block(cfg, sv, prm, pk, gout, need_x, need_y, need_w, eps=None, need_ln=False):
    """The backward of one attention block (``mpg_mab_bwd`` + its weight gradients: queued for the grouped launches inside a
    TrainStep backward, computed at once otherwise) from its ``MABCfg``, ``MABSaved`` and ``MABParams``: (dx rows or None, dy rows
    or None, the six parameter gradients or Nones, lnrows).  ``eps``: of the norms of a ``layer_norm=True`` block; with
    ``need_ln`` the rows for the norms' parameter gradients are produced, lnrows = (dn1, gn1, dn2, gn2), else None."""
    B, L, S, E = cfg.B, cfg.L, cfg.S, cfg.E
    x2, y2, o, z = sv.x2, sv.y2, sv.o, sv.z
    dev = x2.device
    cross = y2 is not None
    dout = gout.reshape(B * L, E).contiguous()
    m = _mab_struct(cfg, x2, y2, sv.ignore, pk, prm, None if sv.n1w is None else (sv.n1w, sv.n1b, sv.n2w, sv.n2b, eps))
    m.save_o, m.save_z, m.save_za = _p(o), _p(z), _p(sv.za)
    m.dout, m.lddout = _p(dout), dout.stride(0)
    dx = torch.empty((B * L, E), device=dev, dtype=torch.float32) if need_x else None
    dy = torch.empty((B * S, E), device=dev, dtype=torch.float32) if (cross and need_y) else None
    m.dx, m.lddx, m.dy, m.lddy = _p(dx), E, _p(dy), E
    dqkv = dq = dkv = dza = du = None
    if need_w:
        if cross:
            dq = torch.empty((B * L, E), device=dev, dtype=torch.float32)
            dkv = torch.empty((B * S, 2 * E), device=dev, dtype=torch.float32)
            m.dq, m.lddq, m.dk, m.dv, m.lddkv = _p(dq), E, _p(dkv), _p(dkv, E), 2 * E
        else:
            dqkv = torch.empty((B * L, 3 * E), device=dev, dtype=torch.float32)
            m.dq, m.lddq, m.dk, m.dv, m.lddkv = _p(dqkv), 3 * E, _p(dqkv, E), _p(dqkv, 2 * E), 3 * E
        dza, du = torch.empty_like(dout), torch.empty_like(dout)
        m.dza, m.du = _p(dza), _p(du)
    elif L > 32 or S > 32:   # (large sets: the waves that own the key tiles read the rows of dza back)
        dza = torch.empty_like(dout)
        m.dza = _p(dza)
    lnrows = None
    if need_ln:
        lnrows = tuple(torch.empty((B * L, E), device=dev, dtype=torch.float32) for _ in range(4))
        m.dn1, m.gn1, m.dn2, m.gn2 = (_p(t) for t in lnrows)
    check(_lib.lib().mpg_mab_bwd(C.byref(m), _stream()), "mpg_mab_bwd")
    # (TrainStep: queued for the grouped launches, added into the flat gradient buffers; nothing happens without ``need_w``)
    pg = ParamGrads(dev_state(dev), prm, (need_w,) * 6)
    if cross:
        pg.gemm(0, 1, dq, x2, rows=slice(0, E))
        pg.gemm(0, 1, dkv, y2, rows=slice(E, None))
    else:
        pg.gemm(0, 1, dqkv, x2)
    pg.gemm(2, 3, dza, o)
    pg.gemm(4, 5, du, z)
    return dx, dy, pg.slots(), lnrows


def sab_chain_forward(x, ignore, H, alpha, ff_act, p_mab, p_ff, training, pks, blocks, save=False):
    """``mpg_mab_chain_fwd``: the self-attention blocks ``blocks`` (their ``MABParams``; ``pks``: their ``PackedMAB`` sets) applied
    to x [B, L, E] one after the other in ONE launch.  Returns (the last block's output [B, L, E], a ``MABSaved`` and a ``MABCfg``
    per block); without ``save`` nothing is kept of o and z."""
    B, L, E = x.shape
    dev = x.device
    c = _lib.MpgMabChain()
    c.n = len(pks)
    inp, saved, cfgs = x.reshape(B * L, E).contiguous(), [], []
    for b, (pk, prm) in enumerate(zip(pks, blocks)):
        cfg = _mab_cfg(dev, B, L, L, E, H, alpha, ff_act, p_mab, p_ff, training)
        out = torch.empty((B * L, E), device=dev, dtype=torch.float32)
        o, z = (torch.empty_like(out), torch.empty_like(out)) if save else (None, None)
        m = _mab_struct(cfg, inp, None, ignore, pk, prm)
        m.out, m.ldo, m.save_o, m.save_z = _p(out), E, _p(o), _p(z)
        c.blk[b] = m
        saved.append(MABSaved(inp, None, ignore, o, z))
        cfgs.append(cfg)
        inp = out
    check(_lib.lib().mpg_mab_chain_fwd(C.byref(c), _stream()), "mpg_mab_chain_fwd")
    return inp.reshape(B, L, E), saved, cfgs


class FusedSABChainFn(torch.autograd.Function):
    """Several self-attention blocks applied one after the other (the SABs of GAPT_G / GAPT_D, gapt/model.py:261-262, :341-342)
    with ONE forward launch (``sab_chain_forward``: a wave keeps its jet's rows in registers from block to block); the backward
    runs block by block (``mpg_mab_bwd``).  ``params``: the blocks' ``MABParams``, one after the other; ``pks``: their
    ``PackedMAB`` sets."""

    @staticmethod
    def forward(ctx, x, ignore, H, alpha, ff_act, p_mab, p_ff, training, pks, *params):
        ctx.blocks = [MABParams(*g) for g in _groups(params, len(MABParams._fields))]
        out, saved, ctx.cfgs = sab_chain_forward(x, ignore, H, alpha, ff_act, p_mab, p_ff, training, pks, ctx.blocks, save=True)
        # the key mask once, then per block what differs: its input rows (the output of the block before), o and z
        ctx.save_for_backward(ignore, *(t for sv in saved for t in (sv.x2, sv.o, sv.z)))
        ctx.pks = pks
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        ignore, *rows = ctx.saved_tensors
        saved = [MABSaved(x2=x2, y2=None, ignore=ignore, o=o, z=z) for x2, o, z in _groups(rows, 3)]
        need_params = _groups(ctx.needs_input_grad[9:], len(MABParams._fields))
        g, all_grads = gout, []
        for b in reversed(range(len(saved))):
            need_x = b > 0 or ctx.needs_input_grad[0]
            g, _, grads, _ = _mab_backward_block(ctx.cfgs[b], saved[b], ctx.blocks[b], ctx.pks[b], g, need_x, False, any(need_params[b]))
            all_grads[:0] = grads
        return (None if g is None else g.reshape(gout.shape), None, None, None, None, None, None, None, None, *all_grads)


class FusedMABFn(torch.autograd.Function):
    """``mab_block`` with a backward: ONE launch each way (``mpg_mab_fwd`` / ``mpg_mab_bwd``).  The forward keeps a ``MABSaved``
    (o, z and, with LayerNorm, za; the backward recomputes the rest); the backward hands the three pre-activation gradients to
    the grouped weight-gradient launches (``TrainStep``) or computes the weight gradients itself.  ``n1w`` ... ``eps``: norm1 /
    norm2 of a block with ``layer_norm=True`` (gapt/model.py:118-120, :131-136), which then run inside the same launches (one wave
    per jet); None without.  The backward then leaves, per row, the gradients with respect to the norms' outputs and those times
    the normalised inputs: their column sums are the norms' parameter gradients (``_colsum_grad``)."""

    @staticmethod
    def forward(ctx, x, y, ignore, Win, bin_, Wo, bo, Wf, bf, n1w, n1b, n2w, n2b, eps, H, alpha, ff_act, p_mab, p_ff, training, pk):
        ctx.params = MABParams(Win, bin_, Wo, bo, Wf, bf)
        ln = None if n1w is None else (n1w, n1b, n2w, n2b, eps)
        out, saved, ctx.cfg, ctx.shared = _mab_run(x, y, ignore, pk, ctx.params, ln, H, alpha, ff_act, p_mab, p_ff, training, True)
        ctx.save_for_backward(*saved)
        ctx.pk, ctx.eps = pk, eps
        # the shared row's gradient is the sum over the jets; the parameter itself: its .grad can take that sum directly
        ctx.seed = x if (ctx.shared and x.is_leaf) else None
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        sv, cfg, need = MABSaved(*ctx.saved_tensors), ctx.cfg, ctx.needs_input_grad
        dx, dy, grads, rows = _mab_backward_block(cfg, sv, ctx.params, ctx.pk, gout, need[0], need[1], any(need[3:9]),
                                                  eps=ctx.eps, need_ln=any(need[9:13]))
        st, gln = dev_state(gout.device), [None] * 4
        if rows is not None:
            # (rows = dn1, gn1, dn2, gn2: dn = the gradient with respect to the norm's output (its bias's), gn = dn times the
            # normalised input (its weight's))
            gln = [_colsum_grad(st, prm, nd, r) for prm, nd, r in zip((sv.n1w, sv.n1b, sv.n2w, sv.n2b), need[9:13],
                                                                      (rows[1], rows[0], rows[3], rows[2]))]
        if ctx.shared and dx is not None:   # (ctx.seed: the row as a leaf parameter, else None -- then it has no .grad to add into)
            dx = _colsum_grad(st, ctx.seed, True, dx)
            dx = None if dx is None else dx.reshape(1, 1, cfg.E)
        elif dx is not None:
            dx = dx.reshape(cfg.B, cfg.L, cfg.E)
        return (dx, None if dy is None else dy.reshape(cfg.B, cfg.S, cfg.E), None, *grads, *gln, None, None, None, None, None, None, None, None)


# ------------------------------------------------------------------------------------- per-jet pieces around the layers
def rank_mask(first_feature: torch.Tensor, labels: torch.Tensor, num_particles: int, out: Optional[torch.Tensor] = None,
              with_ignore: bool = False, ignore_out: Optional[torch.Tensor] = None):
    """mask_c (mpgan/model.py:689-699): [B, N] floats, 1 for the n = int(label * N) particles of each jet with the
    smallest first feature.  ``first_feature`` [B, N] may be a strided view (x[:, :, 0]); one launch.  ``with_ignore``: returns
    (mask, 1 - mask), the second written by the same launch (the key mask of GAPT's attention blocks)."""
    _chk(first_feature, "first_feature")
    B, N = first_feature.shape
    lab = labels[:, -1]
    if lab.dtype != torch.float32:
        lab = lab.float()
    if out is None:
        out = torch.empty((B, N), device=first_feature.device, dtype=torch.float32)
    ign = ignore_out if ignore_out is not None else (torch.empty((B, N), device=first_feature.device, dtype=torch.float32) if with_ignore else None)
    assert out.is_contiguous() and (ign is None or ign.is_contiguous())
    check(_lib.lib().mpg_rank_mask(_p(first_feature), first_feature.stride(0), first_feature.stride(1), _p(lab), lab.stride(0),
                                   B, N, _p(out), _p(ign), _stream()), "mpg_rank_mask")
    return (out, ign) if (with_ignore or ignore_out is not None) else out


def knn_sets(x: torch.Tensor, mask: Optional[torch.Tensor], num_knn: int, self_loops: bool = True):
    """The k-nearest-neighbour graph of MPLayer._getA_knn (mpgan/model.py:319-381) as bit masks [B * N, ceil(N / 32)]
    (int32): bit j of row (b, i) is set when sender j is among the ``num_knn`` nearest neighbours of receiver i
    (zero-masked senders pushed 1e4 times further away, :333-335).  One launch; no gradient (the selection is discrete)."""
    _chk(x, "x")
    B, N, F = x.shape
    x2 = x.reshape(B * N, F)
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    m1 = None if mask is None else mask.reshape(B * N).contiguous()
    nbr = torch.empty((B * N, (N + 31) // 32), device=x.device, dtype=torch.int32)
    check(_lib.lib().mpg_knn_sets(_p(x2), x2.stride(0), _p(m1), B, N, F, num_knn, int(self_loops),
                                  C.c_void_p(nbr.data_ptr()), _stream()), "mpg_knn_sets")
    return nbr


ACT_CODES = {"": 0, "tanh": 1, "sigmoid": 2}


def gen_tail_into(y, mask, act: int, out):
    """out[..., :F] = act(y), out[..., F] = mask - 0.5, written into the caller's [B, N, F+1] buffer (a view with unit
    feature stride is fine); no autograd -- the D step's generator pass runs under ``no_grad`` and lands its jets
    directly in the second half of the discriminator's real+generated batch."""
    B, N, F = y.shape
    y2 = y.reshape(B * N, F)
    if y2.stride(1) != 1:
        y2 = y2.contiguous()
    assert out.shape == (B, N, F + (mask is not None)) and out.stride(2) == 1 and out.stride(0) == N * out.stride(1)
    m1 = None if mask is None else mask.reshape(B * N)
    check(_lib.lib().mpg_gen_tail_fwd(_p(y2), y2.stride(0), _p(m1), _p(out), out.stride(1), B * N, F, act, _stream()),
          "mpg_gen_tail_fwd")
    return out


class GenTailFn(torch.autograd.Function):
    """Final activation + mask column of a generator (MPNet._final_activation / MPGenerator._final_mask,
    mpgan/model.py:533-538, :741-757): out = [act(y) | mask - 0.5], one launch each way."""

    @staticmethod
    def forward(ctx, y, mask, act):
        _chk(y, "y")
        B, N, F = y.shape
        out = torch.empty((B, N, F + (mask is not None)), device=y.device, dtype=torch.float32)
        gen_tail_into(y, mask, act, out)
        ctx.save_for_backward(out)
        ctx.cfg = (B, N, F, act)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        (out,) = ctx.saved_tensors
        B, N, F, act = ctx.cfg
        if dout.stride(2) != 1 or dout.stride(0) != N * dout.stride(1):
            dout = dout.contiguous()
        dy = torch.empty((B * N, F), device=out.device, dtype=torch.float32)
        check(_lib.lib().mpg_gen_tail_bwd(_p(dout), dout.stride(1), _p(out), out.stride(1), _p(dy), F, B * N, F, act, _stream()),
              "mpg_gen_tail_bwd")
        return dy.reshape(B, N, F), None, None


def bridge_fusable(K: int, F: int, E: int) -> bool:
    """Shapes ``GenDiscBridgeFn`` takes (csrc/bridge.hip: sixteen lanes to a row of 64)."""
    return K == 64 and E == 64 and (1 <= F <= 4 or F == 8)


class GenDiscBridgeFn(torch.autograd.Function):
    """The rows between a GAPT generator's last block and the discriminator's first one as ONE launch each way
    (``mpg_bridge_fwd`` / ``mpg_bridge_bwd``):  feat = act1(pre W1' + b1)  (gen's ``final_fc`` + final activation,
    gapt/model.py:263-265), then  e = dropout(LeakyReLU(feat W2' + b2))  (disc's ``input_embedding``, :336-339).

    ``pre`` [Bg, N, K]: the generated jets' rows; ``feat_buf``: None, or a [B, N, F] batch whose first B - Bg jets are real
    ones -- the generated features are written behind them, in place, and every row is embedded (the D step's real +
    generated batch).  Returns (feat [Bg, N, F] -- None with ``feat_buf`` --, e [B, N, E]).  Weight gradients go through the grouped launches like
    ``FusedLinearFn``'s."""

    @staticmethod
    def forward(ctx, pre, W1, b1, feat_buf, W2, b2, act1, act2, alpha, p_drop, training):
        _chk(pre, "pre")
        Bg, N, K = pre.shape
        F, E = W1.shape[0], W2.shape[0]
        pre2 = pre.reshape(Bg * N, K)
        if pre2.stride(1) != 1 or pre2.stride(0) % 4:
            pre2 = pre2.contiguous()
        if feat_buf is None:
            feat = torch.empty((Bg, N, F), device=pre.device, dtype=torch.float32)
        else:
            feat = feat_buf
            assert feat.is_contiguous() and feat.shape[1:] == (N, F) and feat.shape[0] >= Bg
        B = feat.shape[0]
        e = torch.empty((B, N, E), device=pre.device, dtype=torch.float32)
        thr, dscale = drop_params(p_drop) if training else (0, 1.0)
        tag = next_tag(pre.device, "bridge", thr) + TAG_GENERIC
        q = _lib.MpgBridge()
        q.x, q.ldx, q.W1, q.b1, q.act1 = _p(pre2), pre2.stride(0), _p(W1), _p(b1), int(act1)
        q.feat, q.ldf = _p(feat), F
        q.M, q.row0, q.K, q.F, q.E = B * N, (B - Bg) * N, K, F, E
        q.W2, q.b2, q.act2, q.alpha = _p(W2), _p(b2), int(act2), alpha
        q.seed, q.tag, q.thr, q.dscale = _p(seed_tensor(pre.device)), tag, thr, dscale
        q.e, q.lde = _p(e), E
        check(_lib.lib().mpg_bridge_fwd(q, _stream()), "mpg_bridge_fwd")
        ctx.save_for_backward(pre2, W1, W2, feat, e)
        ctx.set_materialize_grads(False)   # (feat usually goes nowhere else: no zeros filled in for its gradient)
        ctx.params = (W1, b1, W2, b2)
        ctx.cfg = (Bg, B, N, K, F, E, int(act1), int(act2), alpha, thr, dscale, tag)
        return (feat if feat_buf is None else None), e   # (a caller's own batch is written in place: nothing new to hand back)

    @staticmethod
    @once_differentiable
    def backward(ctx, gfeat, ge):
        pre2, W1s, W2s, feat, e = ctx.saved_tensors
        W1, b1, W2, b2 = ctx.params
        Bg, B, N, K, F, E, act1, act2, alpha, thr, dscale, tag = ctx.cfg
        need = ctx.needs_input_grad
        if ge is None:   # (only feat was used downstream)
            ge = torch.zeros((B, N, E), device=pre2.device, dtype=torch.float32)
        want1 = need[1] or (b1 is not None and need[2])
        want2 = need[4] or (b2 is not None and need[5])
        M, row0 = B * N, (B - Bg) * N
        dev = pre2.device
        ge2 = ge.reshape(M, E)
        if ge2.stride(1) != 1 or ge2.stride(0) % 4:
            ge2 = ge2.contiguous()
        g2 = torch.empty((M, E), device=dev, dtype=torch.float32) if want2 else None
        g1 = torch.empty((Bg * N, F), device=dev, dtype=torch.float32) if want1 else None
        dx = torch.empty((Bg * N, K), device=dev, dtype=torch.float32) if need[0] else None
        gf = None
        if gfeat is not None and (want1 or need[0]):
            gf = gfeat.reshape(-1, F)[row0:] if gfeat.shape[0] == B else gfeat.reshape(-1, F)
            gf = gf.contiguous()
        q = _lib.MpgBridgeBwd()
        q.ge, q.ldge, q.e, q.lde, q.feat, q.ldf = _p(ge2), ge2.stride(0), _p(e), E, _p(feat), F
        q.gfeat, q.ldgf, q.W1, q.W2 = _p(gf), F, _p(W1s), _p(W2s)
        q.M, q.row0, q.K, q.F, q.E, q.act1, q.act2, q.alpha = M, row0, K, F, E, act1, act2, alpha
        q.seed, q.tag, q.thr, q.dscale = _p(seed_tensor(dev)), tag, thr, dscale
        q.g2, q.ldg2, q.g1, q.ldg1, q.dx, q.lddx = _p(g2), E, _p(g1), F, _p(dx), K
        if want1 or want2 or need[0]:
            check(_lib.lib().mpg_bridge_bwd(q, _stream()), "mpg_bridge_bwd")
        st = dev_state(dev)   # (each layer decides for itself, as two FusedLinearFn nodes would)
        pg1, pg2 = ParamGrads(st, (W1, b1), need[1:3]), ParamGrads(st, (W2, b2), need[4:6])
        pg1.gemm(0, 1, g1, pre2)
        pg2.gemm(0, 1, g2, feat.reshape(M, F))
        return (None if dx is None else dx.reshape(Bg, N, K), *pg1.slots(), None, *pg2.slots(), None, None, None, None, None)


LOSS_CODES = {"ls": 0, "og": 1, "w": 2, "hinge": 3}


def _head_struct(y, mask, w, b, mean, sigmoid, p_drop, training, tag, out, pooled, aux):
    B, N, F = y.shape
    h = _lib.MpgDiscHead()
    h.y, h.ldy, h.mask = _p(y), y.stride(1), _p(mask)
    h.w, h.bias = _p(w), _p(b)
    h.B, h.N, h.F, h.mean, h.sigmoid = B, N, F, int(mean), int(sigmoid)
    thr, dscale = drop_params(p_drop) if training else (0, 1.0)
    h.seed, h.tag, h.thr, h.dscale = _p(seed_tensor(y.device)), tag, thr, dscale
    h.out, h.pooled, h.aux = _p(out), _p(pooled), _p(aux)
    h.loss = -1
    return h


def _head_inputs(y, mask):
    _chk(y, "y")
    B, N, F = y.shape
    if y.stride(2) != 1 or y.stride(0) != N * y.stride(1):
        y = y.contiguous()
    m = None if mask is None else mask.reshape(B, N)
    if m is not None and not m.is_contiguous():
        m = m.contiguous()
    return y, m


class DiscHeadFn(torch.autograd.Function):
    """Discriminator head (mpgan/model.py:812-829 + fnd_layer + :537): out[b] = act(drop(w . pool_i(mask * y) + bias)).
    One launch forward; backward: one launch for dy plus one small reduction for dw / db."""

    @staticmethod
    def forward(ctx, y, mask, w, b, mean, sigmoid, p_drop, training):
        y, m = _head_inputs(y, mask)
        B, N, F = y.shape
        dev = y.device
        out = torch.empty((B,), device=dev, dtype=torch.float32)
        pooled = torch.empty((B, F), device=dev, dtype=torch.float32)
        aux = torch.empty((2 * B,), device=dev, dtype=torch.float32)
        tag = next_tag(dev, "head", drop_params(p_drop)[0] if training else 0) + TAG_GENERIC
        wv = w.reshape(-1)
        h = _head_struct(y, m, wv, b, mean, sigmoid, p_drop, training, tag, out, pooled, aux)
        check(_lib.lib().mpg_disc_head_fwd(C.byref(h), _stream()), "mpg_disc_head_fwd")
        ctx.save_for_backward(y, m, w, b, out, pooled, aux)
        ctx.cfg = (mean, sigmoid, p_drop, training, tag)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        y, m, w, b, out, pooled, aux = ctx.saved_tensors
        mean, sigmoid, p_drop, training, tag = ctx.cfg
        B, N, F = y.shape
        dev = y.device
        h = _head_struct(y, m, w.reshape(-1), b, mean, sigmoid, p_drop, training, tag, out, pooled, aux)
        gout = gout.contiguous()
        h.gout = _p(gout)
        dy = torch.empty((B, N, F), device=dev, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        h.dy, h.ld_dy = _p(dy), F
        need_w = ctx.needs_input_grad[2]   # (w decides for both; a head without bias has one target)
        pg = ParamGrads(dev_state(dev), (w, b), (need_w, need_w and b is not None))
        (tw, tb), h.accumulate = pg.written(lambda: (torch.empty_like(w), None if b is None else torch.empty_like(b)))
        h.dw, h.db = _p(tw), _p(tb)
        check(_lib.lib().mpg_disc_head_bwd(C.byref(h), _stream()), "mpg_disc_head_bwd")
        return dy, None, *pg.slots(), None, None, None, None


def disc_head_loss(y, mask, w, b, *, mean, sigmoid, p_drop, training, loss, n_real, gen_step, count, loss_out,
                   want_dy=True, wgrad=None, targets=None, loss_extra=None):
    """Head forward, the named loss and its gradient in two launches (+ one small reduction), no autograd node:
    returns (out [B], dy [B, N, F] or None).  ``loss_out`` (0-dim tensor) receives the loss value; ``wgrad`` =
    (dw, db) buffers the head's own parameter gradients are ADDED to (the flat .grad views), or None.  ``targets`` [B]: jet b
    is scored against ``targets[b]`` instead of 1 / 0; ``loss_extra`` (one float): added to the loss value (``label_targets``)."""
    y, m = _head_inputs(y, mask)
    B, N, F = y.shape
    dev = y.device
    out = torch.empty((B,), device=dev, dtype=torch.float32)
    pooled = torch.empty((B, F), device=dev, dtype=torch.float32)
    aux = torch.empty((2 * B,), device=dev, dtype=torch.float32)
    terms = torch.empty((B,), device=dev, dtype=torch.float32)
    tag = next_tag(dev, "head", drop_params(p_drop)[0] if training else 0) + TAG_GENERIC
    h = _head_struct(y, m, w.reshape(-1), b, mean, sigmoid, p_drop, training, tag, out, pooled, aux)
    h.loss, h.gen_step, h.n_real, h.inv_count = LOSS_CODES[loss], int(gen_step), n_real, 1.0 / count
    h.terms, h.loss_out = _p(terms), _p(loss_out)
    dy = torch.empty((B, N, F), device=dev, dtype=torch.float32) if want_dy else None
    h.dy, h.ld_dy = _p(dy), F
    if wgrad is not None:
        h.dw, h.db, h.accumulate = _p(wgrad[0]), _p(wgrad[1]), 1
    for t, k, name in ((targets, B, "targets"), (loss_extra, 1, "loss_extra")):
        if t is not None:
            _chk(t, name)
            if not t.is_contiguous() or t.numel() != k or t.device != dev:
                raise ValueError(f"disc_head_loss: {name} must be contiguous with {k} elements on {dev}, got {tuple(t.shape)} on {t.device}")
    h.targets, h.loss_extra = _p(targets), _p(loss_extra)
    check(_lib.lib().mpg_disc_head_loss(C.byref(h), _stream()), "mpg_disc_head_loss")
    return out, dy


# ---- the discriminator head, twice differentiable (the gradient penalty; OPTIONS["gp_chain"]) ---------------------------------
# Per jet, with d = 1 (sum), sum_i m_i + 1e-12 (mean) or N (mean without mask), kappa the output dropout's keep-and-scale:
#   t_i = <w, y_i> ,  S = sum_i m_i t_i ,  s = S / d + b ,  z = kappa s ,  out = phi(z)
# The first- and second-order rules are stated with ``mpg_disc_head_dd`` (include/mpgan_amd.h) and derived in DESIGN.md section 4.
DiscHeadDDSettings = namedtuple("DiscHeadDDSettings", "mean sigmoid p_drop training keep param_grads", defaults=(0.0, True, None, True))
DD_HEAD_MAX_N = 1024    # mpg_disc_head_dd keeps eight floats per particle of a jet in LDS


def gp_head_route(N: int, double_backward: bool, options=None) -> bool:
    """Does a discriminator's single-launch head (``fused_head()``) run as ``DiscHeadDDFn`` inside ``double_backward_route``?  Only
    with the option on (``OPTIONS["gp_chain"]``) and a jet that ``mpg_disc_head_dd`` holds in LDS.  Host only."""
    opt = OPTIONS if options is None else options
    return bool(opt.get("gp_chain") and double_backward and 1 <= N <= DD_HEAD_MAX_N)


class _HeadState:
    __slots__ = ("cpu", "B", "N", "F", "mean", "sigmoid", "thr", "dscale", "tag", "seed_t", "kappa", "param_grads", "mask_shape",
                 "w_shape", "has_bias")


def _head_dd_terms(st, y, m, wv, b):
    # (t [B, N], d [B], c [B], phi'(z), phi''(z)) of the plain-torch form
    t = y @ wv
    S = (t if m is None else m * t).sum(1)
    if not st.mean:
        d = torch.ones_like(S)
    elif m is None:
        d = torch.full_like(S, float(st.N))
    else:
        d = m.sum(1) + 1e-12
    c = S / d if (st.mean and m is not None) else torch.zeros_like(S)
    z = S / d + (0 if b is None else b.reshape(()))
    if st.kappa is not None:
        z = st.kappa * z
    if st.sigmoid:
        o = torch.sigmoid(z)
        return t, d, c, z, o * (1 - o), o * (1 - o) * (1 - 2 * o)
    return t, d, c, z, torch.ones_like(z), torch.zeros_like(z)


def _head_dd_pairwise(m, v, d):
    # v_i d - sum_j m_j v_j as ONE sum of pairwise terms, sum_j m_j (v_i - v_j) + 1e-12 v_i [B, N] (d = sum_j m_j + 1e-12): a jet with one
    # real particle, where the difference is 1e-12 of its terms, keeps its digits (as the kernel forms it)
    return (m.unsqueeze(1) * (v.unsqueeze(2) - v.unsqueeze(1))).sum(2) + 1e-12 * v


def _head_dd_struct(st, y, m, w, b):
    h = _lib.MpgDiscHeadDD()
    h.y, h.ldy, h.mask, h.w, h.bias = _p(y), y.stride(1), _p(m), _p(w), _p(b)
    h.B, h.N, h.F, h.mean, h.sigmoid = st.B, st.N, st.F, int(st.mean), int(st.sigmoid)
    h.seed, h.tag, h.thr, h.dscale = _p(st.seed_t), st.tag, st.thr, st.dscale
    return h


class DiscHeadDDFn(torch.autograd.Function):
    """``DiscHeadFn`` for the gradient penalty: out [B] = phi(kappa (pool_i(m_i <w, y_i>) + b)) with a real-valued mask that takes a
    gradient, twice differentiable.  y [B, N, F]; ``mask`` [B, N] / [B, N, 1] or None; w [1, F] / [F]; b [1] or None; ``settings``: a
    ``DiscHeadDDSettings`` (``keep``: the keep-and-scale [B] of a CPU call, None = no dropout; ``param_grads`` as ``LinearNetFn``'s).
    The forward is ``mpg_disc_head_fwd``; both derivatives are ``mpg_disc_head_dd``.  CPU tensors take the formulas in plain torch."""

    @staticmethod
    def forward(ctx, y, mask, w, b, settings):
        s = settings
        B, N, F = y.shape
        st = _HeadState()
        st.cpu, st.B, st.N, st.F, st.mean, st.sigmoid = not y.is_cuda, B, N, F, bool(s.mean), bool(s.sigmoid)
        st.param_grads, st.mask_shape, st.w_shape, st.has_bias = bool(s.param_grads), None if mask is None else tuple(mask.shape), tuple(w.shape), b is not None
        ctx.st = st
        ctx.save_for_backward(y, mask, w, b)
        if st.cpu:
            st.kappa = s.keep
            z = _head_dd_terms(st, y, None if mask is None else mask.reshape(B, N), w.reshape(-1), b)[3]
            return torch.sigmoid(z) if st.sigmoid else z
        if N > DD_HEAD_MAX_N:
            raise ValueError(f"DiscHeadDDFn: at most {DD_HEAD_MAX_N} particles per jet, got {N}")
        y2, m = _head_inputs(y, mask)
        dev = y.device
        st.thr, st.dscale = drop_params(s.p_drop) if s.training else (0, 1.0)
        st.seed_t, st.tag = seed_tensor(dev), next_tag(dev, "head_dd", st.thr) + TAG_GENERIC
        out = torch.empty((B,), device=dev, dtype=torch.float32)
        aux = torch.empty((2 * B,), device=dev, dtype=torch.float32)
        h = _head_struct(y2, m, w.reshape(-1), b, st.mean, st.sigmoid, s.p_drop, s.training, st.tag, out, None, aux)
        check(_lib.lib().mpg_disc_head_fwd(C.byref(h), _stream()), "mpg_disc_head_fwd")
        return out

    @staticmethod
    def backward(ctx, g):
        y, mask, w, b = ctx.saved_tensors
        need, st = ctx.needs_input_grad, ctx.st
        again = torch.is_grad_enabled()
        flags = (need[0], mask is not None and need[1], (need[2] or need[3]) and (st.param_grads or not again), again)
        return (*DiscHeadVJPFn.apply(g, y, mask, w, b, st, flags), None)


class DiscHeadVJPFn(torch.autograd.Function):
    """The first derivative of ``DiscHeadDDFn`` as a function of (g, y, mask, w, b): (y_bar, m_bar, w_bar, b_bar).  Its own backward
    takes cotangents U on y_bar and mu on m_bar (an absent one is zero) -- one on a parameter gradient raises -- and is once
    differentiable."""

    @staticmethod
    def forward(ctx, g, y, mask, w, b, st, flags):
        need_y, need_m, need_w, again = flags
        ctx.st, ctx.flags, ctx.g_shape = st, flags, tuple(g.shape)
        ctx.set_materialize_grads(False)
        B, N, F = st.B, st.N, st.F
        if st.cpu:
            ctx.save_for_backward(g, y, mask, w, b)
            m = None if mask is None else mask.reshape(B, N)
            t, d, c, z, d1, _ = _head_dd_terms(st, y, m, w.reshape(-1), b)
            gh = g.reshape(B) * d1 * (1 if st.kappa is None else st.kappa)
            cy = (gh / d).unsqueeze(1) * (torch.ones_like(t) if m is None else m)
            ybar = cy.unsqueeze(2) * w.reshape(-1) if need_y else None
            mbar = None
            if need_m:
                tau = _head_dd_pairwise(m, t, d) / d.unsqueeze(1) if st.mean else t      # t_i - c
                mbar = ((gh / d).unsqueeze(1) * tau).reshape(st.mask_shape)
            wbar = (cy.unsqueeze(2) * y).sum((0, 1)).reshape(st.w_shape) if need_w else None
            bbar = gh.sum().reshape(b.shape) if (need_w and b is not None) else None
            return ybar, mbar, wbar, bbar
        dev = y.device
        y2, m = _head_inputs(y, mask)
        g1 = g.reshape(B).float().contiguous()
        wv = w.reshape(-1)
        ctx.save_for_backward(g1, y2, m, wv, b)
        h = _head_dd_struct(st, y2, m, wv, b)
        h.mode, h.g = 0, _p(g1)
        ybar = torch.empty((B, N, F), device=dev, dtype=torch.float32) if need_y else None
        mbar = torch.empty((B, N), device=dev, dtype=torch.float32) if need_m else None
        part = torch.empty((B, F + 1), device=dev, dtype=torch.float32) if need_w else None
        wbar = torch.empty((F,), device=dev, dtype=torch.float32) if need_w else None
        bbar = torch.empty((1,), device=dev, dtype=torch.float32) if (need_w and b is not None) else None
        h.gy, h.ld_gy, h.gm, h.part, h.gw, h.gb = _p(ybar), F, _p(mbar), _p(part), _p(wbar), _p(bbar)
        check(_lib.lib().mpg_disc_head_dd(C.byref(h), _stream()), "mpg_disc_head_dd")
        return (ybar, None if mbar is None else mbar.reshape(st.mask_shape), None if wbar is None else wbar.reshape(st.w_shape),
                None if bbar is None else bbar.reshape(b.shape))

    @staticmethod
    @once_differentiable
    def backward(ctx, U, mu, gw_, gb_):
        if gw_ is not None or gb_ is not None:
            raise RuntimeError("DiscHeadVJPFn: a cotangent arrived on a parameter-gradient output; the second-order rule covers the "
                               "input gradient and the mask gradient only")
        st = ctx.st
        if not ctx.flags[3]:
            raise RuntimeError("DiscHeadVJPFn: the first derivative was taken without create_graph=True; there is nothing to differentiate again")
        B, N, F = st.B, st.N, st.F
        n_g, n_y, n_m, n_w, n_b = ctx.needs_input_grad[:5]
        if st.cpu:
            g, y, mask, w, b = ctx.saved_tensors
            m = None if mask is None else mask.reshape(B, N)
            wv = w.reshape(-1)
            t, d, c, z, d1, d2 = _head_dd_terms(st, y, m, wv, b)
            kap = torch.ones_like(z) if st.kappa is None else st.kappa
            mm = st.mean and m is not None
            m1 = torch.ones_like(t) if m is None else m
            a = torch.zeros_like(t) if U is None else U @ wv
            u = torch.zeros_like(t) if mu is None else mu.reshape(B, N)
            Q = u.sum(1) if mm else torch.zeros_like(z)
            g1 = g.reshape(B)
            gh = g1 * d1 * kap
            col = lambda v: v.unsqueeze(1)
            # under the mean with a mask the three differences of the rule come as single sums of pairwise terms (_head_dd_pairwise):
            # tc_i = t_i - c,  al_i = a_i d - sum_j m_j a_j,  be_i = mu_i d - Q m_i
            tc = _head_dd_pairwise(m, t, d) / col(d) if mm else t
            Pt = (u * tc).sum(1)                                       # sum_i mu_i (t_i - c)
            R = ((m1 * a).sum(1) + Pt) / d
            H = g1 * kap * kap * d2 * R
            if mm:
                be = (col(u).transpose(1, 2) * col(m) - col(u) * col(m).transpose(1, 2)).sum(2) + 1e-12 * u
                cy = col(H / d) * m1 + col(gh / d / d) * be
                gm = col(H / d) * tc + col(gh / d / d) * (_head_dd_pairwise(m, a, d) - col(Pt) - col(Q) * tc)
            else:
                cy = col(H / d) * m1 + col(gh / d) * u
                gm = col(H / d) * tc + col(gh / d) * a
            gw = (cy.unsqueeze(2) * y).sum((0, 1))
            if U is not None:
                gw = gw + ((col(gh / d) * m1).unsqueeze(2) * U).sum((0, 1))
            return ((kap * d1 * R).reshape(g.shape), cy.unsqueeze(2) * wv, None if mask is None else gm.reshape(st.mask_shape),
                    gw.reshape(st.w_shape), None if b is None else H.sum().reshape(b.shape), None, None)
        g1, y2, m, wv, b = ctx.saved_tensors
        dev = y2.device
        h = _head_dd_struct(st, y2, m, wv, b)
        h.mode, h.g = 1, _p(g1)
        U2 = None
        if U is not None:
            U2 = U.reshape(B, N, F).float()
            if U2.stride(2) != 1 or U2.stride(0) != N * U2.stride(1):
                U2 = U2.contiguous()
        mu1 = None if (mu is None or m is None) else mu.reshape(B, N).float().contiguous()
        h.U, h.ldu, h.mu = _p(U2), F if U2 is None else U2.stride(1), _p(mu1)
        want_w = n_w or (n_b and b is not None)
        gg = torch.empty((B,), device=dev, dtype=torch.float32) if n_g else None
        gy = torch.empty((B, N, F), device=dev, dtype=torch.float32) if n_y else None
        gm = torch.empty((B, N), device=dev, dtype=torch.float32) if (n_m and m is not None) else None
        part = torch.empty((B, F + 1), device=dev, dtype=torch.float32) if want_w else None
        gw = torch.empty((F,), device=dev, dtype=torch.float32) if n_w else None
        gb = torch.empty((1,), device=dev, dtype=torch.float32) if (n_b and b is not None) else None
        h.gy, h.ld_gy, h.gm, h.gg, h.part, h.gw, h.gb = _p(gy), F, _p(gm), _p(gg), _p(part), _p(gw), _p(gb)
        check(_lib.lib().mpg_disc_head_dd(C.byref(h), _stream()), "mpg_disc_head_dd")
        return (None if gg is None else gg.reshape(ctx.g_shape), gy, None if gm is None else gm.reshape(st.mask_shape),
                None if gw is None else gw.reshape(st.w_shape),
                None if gb is None else gb.reshape(b.shape), None, None)


class BatchNormFn(torch.autograd.Function):
    """nn.BatchNorm1d in training mode over the rows of x [M, F] (LinearNet's optional normalisation, mpgan/model.py:58-60,
    :80-81) on ``mpg_batchnorm_*``; returns (y, batch mean, biased batch variance) -- the caller keeps the running
    statistics (``LinearNet._bn``)."""

    @staticmethod
    def forward(ctx, x, w, b, eps):
        _chk(x, "x")
        x2 = x.contiguous()
        M, F = x2.shape
        nchunk = max(1, min(256, M // 64))
        part = torch.empty((nchunk, F), device=x.device, dtype=torch.float32)
        mean, var = (torch.empty(F, device=x.device, dtype=torch.float32) for _ in range(2))
        check(_lib.lib().mpg_batchnorm_stats(_p(x2), x2.stride(0), M, F, _p(part), nchunk, _p(mean), _p(var), _stream()),
              "mpg_batchnorm_stats")
        y = torch.empty_like(x2)
        check(_lib.lib().mpg_batchnorm_apply(_p(x2), x2.stride(0), _p(mean), _p(var), _p(w), _p(b), eps, _p(y), y.stride(0), M, F,
                                             _stream()), "mpg_batchnorm_apply")
        ctx.save_for_backward(x2, w, mean, var)
        ctx.eps, ctx.params = eps, (w, b)
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gm, _gv):
        x2, w, mean, var = ctx.saved_tensors
        M, F = x2.shape
        g2 = g.contiguous()
        nchunk = max(1, min(256, M // 64))
        part = torch.empty((2 * nchunk, F), device=g.device, dtype=torch.float32)
        sums = torch.empty(2 * F, device=g.device, dtype=torch.float32)
        dx = torch.empty_like(x2) if ctx.needs_input_grad[0] else None
        # (a frozen norm -- the discriminator's inside train_G -- keeps its .grad buffer as the optimizer launch left it: cleared;
        # the launch then writes its two sums into scratch, as it always has)
        pg = ParamGrads(dev_state(g.device), ctx.params, (ctx.needs_input_grad[1] or ctx.needs_input_grad[2],) * 2)
        (dw, db), acc = pg.written(lambda: (sums.new_empty(F), sums.new_empty(F)), scratch=True)
        check(_lib.lib().mpg_batchnorm_bwd(_p(g2), g2.stride(0), _p(x2), x2.stride(0), _p(mean), _p(var), _p(w), ctx.eps, _p(part), nchunk,
                                           _p(sums), _p(dx), F, _p(dw), _p(db), acc, M, F, _stream()), "mpg_batchnorm_bwd")
        return dx, *pg.slots(), None


def batchnorm_eval(x, w, b, mean, var, eps):
    """BatchNorm1d with given (running) statistics: one elementwise launch, no gradient bookkeeping of its own."""
    x2 = x.contiguous()
    M, F = x2.shape
    y = torch.empty_like(x2)
    check(_lib.lib().mpg_batchnorm_apply(_p(x2), x2.stride(0), _p(mean), _p(var), _p(w), _p(b), eps, _p(y), y.stride(0), M, F, _stream()),
          "mpg_batchnorm_apply")
    return y


class LayerNormFn(torch.autograd.Function):
    """nn.LayerNorm over the last dimension (GAPT's MAB.norm1 / norm2, gapt/model.py:118-120, :131-136): one launch
    forward, one launch + a fixed-order reduction of the weight / bias gradients backward."""

    @staticmethod
    def forward(ctx, x, w, b, eps):
        _chk(x, "x")
        shp = x.shape
        E = shp[-1]
        x2 = x.reshape(-1, E)
        if x2.stride(1) != 1:
            x2 = x2.contiguous()
        M = x2.shape[0]
        y = torch.empty((M, E), device=x.device, dtype=torch.float32)
        stats = torch.empty((M, 2), device=x.device, dtype=torch.float32)
        check(_lib.lib().mpg_layernorm_fwd(_p(x2), x2.stride(0), _p(w), _p(b), _p(y), E, _p(stats), M, E, eps, _stream()),
              "mpg_layernorm_fwd")
        ctx.save_for_backward(x2, w, stats)
        ctx.params = (w, b)
        ctx.shp = shp
        return y.reshape(shp)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x2, w, stats = ctx.saved_tensors
        M, E = x2.shape
        g2 = g.reshape(M, E)
        if g2.stride(1) != 1:
            g2 = g2.contiguous()
        dx = torch.empty((M, E), device=g.device, dtype=torch.float32)
        nwaves = 4 * min(256, (M + 3) // 4)
        part = torch.empty((nwaves, 2, E), device=g.device, dtype=torch.float32)
        # (a frozen norm -- the discriminator's inside train_G -- forms no parameter gradient at all: its .grad buffer was cleared by the
        # optimizer launch before and must stay clean for the next train_D, TrainStep has no zero_grad there)
        pg = ParamGrads(dev_state(g.device), ctx.params, (ctx.needs_input_grad[1] or ctx.needs_input_grad[2],) * 2)
        (tw, tb), acc = pg.written(lambda: (torch.empty_like(w), torch.empty_like(w)))
        check(_lib.lib().mpg_layernorm_bwd(_p(g2), g2.stride(0), _p(x2), x2.stride(0), _p(w), _p(stats), _p(dx), E, _p(part),
                                           nwaves, _p(tw), _p(tb), acc, M, E, _stream()), "mpg_layernorm_bwd")
        return dx.reshape(ctx.shp), *pg.slots(), None
