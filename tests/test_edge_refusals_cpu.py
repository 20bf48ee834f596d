"""CPU: the return codes of the five edge entry points' refusals, and the order in which the checks are made.

Every case returns before the first HIP call (no pointer is dereferenced, nothing is launched), so the codes are pinned on a
machine without a GPU."""
import ctypes

import pytest

NA = -100   # MPG_FN_NA
PTR = 0x1000   # "any non-null value": never dereferenced on these paths


def _desc(cls, **kw):
    d = cls()   # ctypes zero-initialises
    base = dict(B=2, N=5, alpha=0.2, f16=1)
    if hasattr(d, "SC"):
        base["SC"] = 1
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


def _fwd(**kw):
    from mpgan_amd import _lib
    return _lib.lib().mpg_edge_fwd(ctypes.byref(_desc(_lib.MpgEdgeFwd, **kw)), None)


def _fwd_fn(chain=None, **kw):
    from mpgan_amd import _lib
    c = _lib.MpgChain()
    for k, v in dict(alpha=0.2, f16=1, **(chain or {})).items():
        setattr(c, k, v)
    return _lib.lib().mpg_edge_fwd_fn(ctypes.byref(_desc(_lib.MpgEdgeFwd, **kw)), ctypes.byref(c), None, None)


def _bwd(**kw):
    from mpgan_amd import _lib
    kw = dict(dict(sign3=PTR, stageE2=PTR), **kw)
    return _lib.lib().mpg_edge_bwd(ctypes.byref(_desc(_lib.MpgEdgeBwd, **kw)), None)


def _bwd_fn(**kw):
    from mpgan_amd import _lib
    kw = dict(dict(sign3=PTR, stageE2=PTR), **kw)
    cdx = _lib.MpgChain()
    return _lib.lib().mpg_edge_bwd_fn(ctypes.byref(_desc(_lib.MpgEdgeBwd, **kw)), ctypes.byref(cdx), None, None)


def _dw(**kw):
    from mpgan_amd import _lib
    kw = dict(dict(nwg=4, gexp=PTR), **kw)
    return _lib.lib().mpg_edge_dw(ctypes.byref(_desc(_lib.MpgEdgeDw, **kw)), None)


CASES = [
    (_fwd, dict(B=0), -1),
    (_fwd, dict(alpha=2.0), -4),
    (_fwd, dict(f16=0), -8),
    (_fwd, dict(two_term=2), -8),
    (_fwd, dict(N=1000), -6),
    # the border of the list: 161 senders in one chunk are refused, in two chunks they get past the list check (index mode) --
    # and, with a fault the entry checks later, still return before any launch
    (_fwd, dict(N=161, SC=1), -6),
    (_fwd, dict(N=161, SC=1, es=PTR), -6),
    (_fwd, dict(N=161, SC=2, es=PTR), -3),              # wq null
    (_fwd, dict(N=160, SC=1, es=PTR), -3),
    (_fwd, dict(es=PTR), -3),                           # wq null
    (_fwd, dict(B=100000, N=150, stageE2=PTR), -7),
    (_fwd, dict(B=0, alpha=2.0), -1),                   # two faults at once: the order of the checks
    (_fwd, dict(alpha=2.0, f16=0), -4),
    (_fwd_fn, dict(B=0), -1),
    (_fwd_fn, dict(alpha=2.0), -4),
    (_fwd_fn, dict(f16=0), -8),
    (_fwd_fn, dict(es=PTR), NA),
    (_fwd_fn, dict(SC=2), NA),                          # sender chunks without tickets
    (_fwd_fn, dict(chain=dict(nlayers=2)), NA),
    (_bwd, dict(B=0), -1),
    (_bwd, dict(sign3=None), -3),
    (_bwd, dict(alpha=-1.0), -4),
    (_bwd, dict(f16=0), -8),
    (_bwd, dict(N=1000), -6),
    (_bwd, dict(N=161, SC=1), -6),
    (_bwd, dict(N=161, SC=1, stageZ2=PTR), -6),
    (_bwd, dict(N=161, SC=2, stageZ2=PTR), -9),         # past the list check: gexp null
    (_bwd, dict(N=160, SC=1, stageZ2=PTR), -9),
    (_bwd, dict(B=100000, N=150), -7),
    (_bwd, dict(stageZ2=PTR), -9),                      # gexp null
    (_bwd, dict(es=PTR), -3),                           # wq null
    (_bwd, dict(es=PTR, wq=PTR, des=PTR, daq=PTR, N=120), -6),   # the 116-sender limit of the edge-scalar kernel
    (_bwd_fn, dict(B=0), -1),
    (_bwd_fn, dict(sign3=None), -3),
    (_bwd_fn, dict(f16=0), -8),
    (_bwd_fn, dict(stageZ2=PTR), -9),                   # gexp null
    (_bwd_fn, dict(SC=2), NA),
    (_bwd_fn, dict(N=33), NA),
    (_bwd_fn, dict(), NA),                              # a zeroed dx chain is none of its shapes
    (_dw, dict(B=0), -1),
    (_dw, dict(nwg=0), -1),
    (_dw, dict(f16=0), -8),
    (_dw, dict(gexp=None), -9),
    (_dw, dict(B=64, N=30, nwg=1), -5),
]


@pytest.mark.parametrize("entry,kw,code", CASES, ids=["%s-%s" % (e.__name__.strip("_"), "-".join("%s=%s" % i for i in k.items()) or "plain")
                                                      for e, k, _ in CASES])
def test_edge_entry_refusal_codes(entry, kw, code):
    assert entry(**kw) == code
