"""Bitwise A/B of the attention backward between two builds: dumps the raw bf16 output of tld_debug_attention_bwd on the random family of
tests/test_gpu_attn_bwd_classes.py, at every case of its table, for the library selected by TLD_LIB.

    TLD_LIB=<lib.so> python tools/attn_bwd_ab_check.py a.npy;  python tools/attn_bwd_ab_check.py b.npy;  python tools/attn_bwd_ab_check.py a.npy b.npy"""
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "tests")]

if len(sys.argv) == 3:
    a, b = np.load(sys.argv[1]), np.load(sys.argv[2])
    same = a.shape == b.shape and bool((a == b).all())
    print(f"{sys.argv[1]} vs {sys.argv[2]}: {a.size} bf16 values, " + ("bitwise identical" if same else f"{int((a != b).sum()) if a.shape == b.shape else 'shape'} differ"))
    sys.exit(0 if same else 1)
import test_gpu_attn_bwd_classes as T
T.dump_random(sys.argv[1])
print(os.path.basename(os.environ.get("TLD_LIB", "default")), "dumped", sys.argv[1])
