"""CPU: the return codes of the three attention-block entry points' refusals, and the order in which the checks are made.

Every case returns before the first HIP call (no pointer is dereferenced, nothing is launched), so the codes are pinned on a
machine without a GPU."""
import ctypes

import pytest

PTR, PTR2, PTR3 = 0x1000, 0x2000, 0x3000   # "any non-null value": never dereferenced on these paths
NAN = float("nan")


def _block(**kw):
    """A self-attention block every check accepts (x = y, E = 32, two heads)."""
    from mpgan_amd import _lib
    p = _lib.MpgMab()   # ctypes zero-initialises
    base = dict(x=PTR, y=PTR, ldx=32, ldy=32, ldo=32, out=PTR2, B=2, L=4, S=4, E=32, H=2, alpha=0.2)
    base.update(kw)
    for k, v in base.items():
        setattr(p, k, v)
    return p


def _fwd(**kw):
    from mpgan_amd import _lib
    return _lib.lib().mpg_mab_fwd(ctypes.byref(_block(**kw)), None)


def _bwd(**kw):
    from mpgan_amd import _lib
    kw = dict(dict(dout=PTR, save_z=PTR, lddout=32), **kw)
    return _lib.lib().mpg_mab_bwd(ctypes.byref(_block(**kw)), None)


LN = dict(ln1_w=PTR, ln1_b=PTR, ln2_w=PTR, ln2_b=PTR, ln_eps=1e-5)   # a complete layer_norm=True forward
LN_BWD = dict(LN, save_za=PTR)                                       # ... and backward (no parameter-gradient rows)


def _chain(n=2, blocks=None):
    """A chain of ``n`` blocks every check accepts, each reading what the one before it writes; blocks: {index: fields to change}."""
    from mpgan_amd import _lib
    c = _lib.MpgMabChain()
    c.n = n
    ptrs = [PTR, PTR2, PTR3, 0x4000, 0x5000]
    for b in range(min(max(n, 1), _lib.MAB_CHAIN_MAX)):
        kw = dict(x=ptrs[b], y=ptrs[b], out=ptrs[b + 1])
        kw.update((blocks or {}).get(b, {}))
        c.blk[b] = _block(**kw)
    return _lib.lib().mpg_mab_chain_fwd(ctypes.byref(c), None)


SHAPE = [   # mab_check: what mpg_mab_fwd and mpg_mab_bwd ask first, in this order
    (dict(B=0), -1),
    (dict(L=0), -1),
    (dict(S=0), -1),
    (dict(L=161), -1),
    (dict(S=161), -1),
    (dict(E=48, H=3), -2),
    (dict(E=128, H=8), -2),
    (dict(H=4), -2),
    (dict(E=64, H=2), -2),
    (dict(alpha=-0.1), -4),
    (dict(alpha=1.5), -4),
    (dict(alpha=NAN), -4),
    (dict(ldx=30), -3),
    (dict(ldy=34), -3),
    (dict(ldo=33), -3),
    (dict(B=0, E=48), -1),                              # two faults at once: the order of the checks
    (dict(L=161, alpha=2.0), -1),
    (dict(H=4, alpha=NAN), -2),
    (dict(E=48, ldx=30), -2),
    (dict(alpha=2.0, ldo=33), -4),
]

CASES = [(_fwd, kw, code) for kw, code in SHAPE] + [(_bwd, kw, code) for kw, code in SHAPE] + [
    # mab_ln_check, forward: ln1_w set brings the other three and a positive eps
    (_fwd, dict(LN, ln2_w=None), -6),
    (_fwd, dict(LN, ln_eps=0.0), -6),
    (_fwd, dict(LN, ln_eps=NAN), -6),
    (_fwd, dict(LN, ln1_b=None), -6),
    (_fwd, dict(LN, ln2_b=None), -6),
    (_fwd, dict(LN, ln2_w=None, ldx=30), -3),           # the shape checks come first
    (_fwd, dict(LN, ln2_w=None, alpha=2.0), -4),
    # mpg_mab_bwd behind the shape checks: its own arguments, the gradients' leading dimensions, then the norms
    (_bwd, dict(dout=None), -5),
    (_bwd, dict(save_z=None), -5),
    (_bwd, dict(dk=PTR), -5),
    (_bwd, dict(dv=PTR), -5),
    (_bwd, dict(lddout=30), -3),
    (_bwd, dict(dq=PTR, lddq=30), -3),
    (_bwd, dict(dk=PTR, dv=PTR, lddkv=30), -3),
    (_bwd, dict(dx=PTR, lddx=30), -3),
    (_bwd, dict(dy=PTR, lddy=30), -3),
    (_bwd, dict(dout=None, ldx=30), -3),                # order: shape, own arguments, leading dimensions, norms
    (_bwd, dict(dout=None, lddout=30), -5),
    (_bwd, dict(LN_BWD, ln2_w=None, lddout=30), -3),
    (_bwd, dict(LN_BWD, ln2_w=None, dk=PTR), -5),
    (_bwd, dict(LN_BWD, ln2_w=None), -6),
    (_bwd, dict(LN_BWD, ln_eps=0.0), -6),
    (_bwd, dict(LN_BWD, save_za=None), -6),
    (_bwd, dict(LN_BWD, dn1=PTR), -6),                  # the rows of the norms' parameter gradients: all four or none
    (_bwd, dict(LN_BWD, gn1=PTR), -6),
    (_bwd, dict(LN_BWD, dn1=PTR, gn1=PTR, dn2=PTR), -6),
    (_bwd, dict(LN_BWD, dn1=PTR, gn1=PTR, gn2=PTR), -6),
    # mpg_mab_chain_fwd: the number of blocks, the first block's shape, then block by block
    (_chain, dict(n=0), -1),
    (_chain, dict(n=-1), -1),
    (_chain, dict(n=5), -1),
    (_chain, dict(blocks={0: dict(B=0)}), -1),
    (_chain, dict(blocks={0: dict(E=48)}), -2),
    (_chain, dict(blocks={0: dict(alpha=NAN)}), -4),
    (_chain, dict(blocks={0: dict(ldo=33)}), -3),
    (_chain, dict(blocks={0: dict(L=33, S=33), 1: dict(L=33, S=33)}), -1),
    (_chain, dict(n=5, blocks={0: dict(E=48)}), -1),    # the order of the checks
    (_chain, dict(blocks={0: dict(L=33, S=33, E=48)}), -2),
    (_chain, dict(blocks={0: dict(y=PTR3)}), -2),
    (_chain, dict(blocks={0: dict(S=5)}), -2),
    (_chain, dict(blocks={0: dict(out=None)}), -2),
    (_chain, dict(blocks={0: dict(ln1_w=PTR)}), -2),
    (_chain, dict(blocks={1: dict(y=PTR3)}), -2),
    (_chain, dict(blocks={1: dict(B=3)}), -2),
    (_chain, dict(blocks={1: dict(L=5, S=5)}), -2),
    (_chain, dict(blocks={1: dict(S=5)}), -2),
    (_chain, dict(blocks={1: dict(E=64, H=4)}), -2),
    (_chain, dict(blocks={1: dict(H=4)}), -2),
    (_chain, dict(blocks={1: dict(ignore=PTR3)}), -2),
    (_chain, dict(blocks={1: dict(seed=PTR3)}), -2),
    (_chain, dict(blocks={1: dict(wscale=2.0)}), -2),
    (_chain, dict(blocks={1: dict(ascale=2.0)}), -2),
    (_chain, dict(blocks={1: dict(out=None)}), -2),
    (_chain, dict(blocks={1: dict(ldo=33)}), -2),
    (_chain, dict(blocks={1: dict(ln1_w=PTR)}), -2),
    (_chain, dict(blocks={1: dict(x=PTR3, y=PTR3)}), -2),   # not the rows the block before it writes
    (_chain, dict(blocks={1: dict(ldx=64)}), -2),
    (_chain, dict(blocks={1: dict(alpha=2.0)}), -4),
    (_chain, dict(blocks={1: dict(alpha=NAN)}), -4),
    (_chain, dict(blocks={1: dict(alpha=2.0, B=3)}), -2),   # a block's mismatch is asked before its alpha
    (_chain, dict(n=3, blocks={1: dict(alpha=2.0), 2: dict(B=3)}), -4),   # ... and block 1 before block 2
]


def _id(entry, kw):
    def one(k, v):
        if isinstance(v, dict):
            return "%s[%s]" % (k, ",".join(one(a, b) for a, b in v.items()))
        return "%s=%s" % (k, v)
    # (of a layer-norm case, only what differs from the complete set)
    return "%s-%s" % (entry.__name__.strip("_"), "-".join(one(k, v) for k, v in kw.items() if LN.get(k) != v) or "ln")


@pytest.mark.parametrize("entry,kw,code", CASES, ids=[_id(e, k) for e, k, _ in CASES])
def test_mab_entry_refusal_codes(entry, kw, code):
    assert entry(**kw) == code
