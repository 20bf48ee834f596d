#!/usr/bin/env python3
"""Phase timing of mpg_mab_fwd / mpg_mab_bwd from a diagnostic build (s_memtime stamps of workgroup 0; each direction's unit,
   csrc/mab_fwd.hip and csrc/mab_bwd.hip (sets of up to 32 tokens), keeps its own stamps and its own entry point to read them):
   MPG_HIPCC_FLAGS="-fno-slp-vectorize -DMPG_MABSTAMP" python -c "from mpgan_amd import _lib; _lib.build(force=True)"
   python tools/mab_stamps.py            (then rebuild without the flag)"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mpgan_amd import _lib
from mpgan_amd.gapt import SAB
B = int(os.environ.get("MAB_B", "512"))
blk = SAB(embed_dim=64, ff_layers=[], final_linear=False, num_heads=4, layer_norm=False, dropout_p=0.0,
          linear_args={"leaky_relu_alpha": 0.2, "dropout_p": 0.0, "batch_norm": False, "spectral_norm": False}).cuda()
x = torch.randn(B, 30, 64, device="cuda")
with torch.no_grad():
    for _ in range(3):
        blk(x, None)
xg = x.clone().requires_grad_(True)
for _ in range(3):
    blk(xg, None).sum().backward()
torch.cuda.synchronize()
lib = C.CDLL(_lib.LIBPATH)
fbuf, bbuf = (C.c_ulonglong * 64)(), (C.c_ulonglong * 64)()   # [wave][stamp] of the last forward / backward launch: up to eight waves
assert lib.mpg_debug_mab_fwd_stamps(fbuf) == 0 and lib.mpg_debug_mab_bwd_stamps(bbuf) == 0
mode = os.environ.get("MPG_MAB_SPLIT", "1")
split = mode != "0" and B <= 512                      # two waves per jet both ways (mab_fwd2_kernel / mab_bwd2_kernel)
fwd8 = mode != "0" and 512 < B <= 1024                # ... the forward alone, eight waves to a workgroup
ONE = ["start", "weights in LDS", "rows loaded", "attention done", "out-projection done", "stored"]
# (waves 0, 1 = the first jet's pair; stamp 2 is not written: q k v and the attention are one function, attn_tile)
names = ["start", "weights in LDS", "-", "q k v + attention", "o exchanged", "z", "z exchanged", "stored"] if split or fwd8 else ONE
bnames = (["start", "weights in LDS", "du", "du exchanged", "dza exchanged", "attention", "dq dk dv exchanged", "stored"] if split else
          ["start", "weights in LDS", "rows loaded", "feed-forward half done", "attention + input gradients done", "stored"])
for w in range(8 if fwd8 else 4):
    st = [fbuf[w * 8 + i] for i in range(len(names))]
    print("forward  wave", w, " ".join(f"{names[i]}={st[i] - st[0]}" for i in range(1, len(names)) if st[i]))
for w in range(4):
    st = [bbuf[w * 8 + i] for i in range(len(bnames))]
    print("backward wave", w, " ".join(f"{bnames[i]}={st[i] - st[0]}" for i in range(1, len(bnames)) if st[i]))
