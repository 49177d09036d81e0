"""Diagnostic: where wave 0 spends its cycles inside dense_lu, and wave 7 in the in-wave finish of the last 16 pivots behind it
(library built by `tools/diag_dense.sh stamps`, or `stampsN` with DIAG_LIB=libdiag_stampsN.so for MISTRA_DENSE_TILE_FROM=N).  The tile steps' sections are
stamped by the wave that sets their pace: the diagonal tile's owner (chain, barrier 1), wave 4 (the L panel's solve, barrier 2, the stores) and
wave 7 (the MFMAs)."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _diag import use_diag_lib
use_diag_lib(os.environ.get('DIAG_LIB', 'libdiag_stamps.so'))
import numpy as np
from mistra_amd import chem
from mistra_amd.workload import make_batch
chem.init(0)
var, fix, rconst = make_batch('tot', 0, 512, 'cpu')
res = chem.integrate('tot', var.numpy(), fix.numpy(), rconst.numpy())
out = (C.c_ulonglong * 24)()
assert chem.lib().mistra_diag_dense_stamps(out, 1) == 0
calls, panels = out[9], out[8]
names = {6: 'table loads land', 7: 'LU program (VM)', 10: 'scaling pass', 0: 'load+schur', 1: 'scale L', 2: 'publish+barrier', 3: 'chain (wave 0)', 4: 'barrier 2', 5: 'mfma update', 12: 'panel loop', 11: 'dense_lu (+ a final barrier)',
         13: 'finish: to rows + chain', 14: 'finish: stores'}
print('dense_lu calls', calls, 'panels', panels)
for k, n in names.items():
    print('%-18s %8.0f cycles per call' % (n, out[k] / calls), '(wave 7; %.0f per pivot)' % (out[k] / calls / 16) if k == 13 else '(wave 7)' if k == 14 else '' if k in (0, 1, 6, 7, 10, 11, 12) or not panels else '(%.0f per panel)' % (out[k] / panels))
steps = out[23]
if steps:
    tiles = {16: 'tile: to rows + chain', 17: 'tile: rows to LDS', 18: 'tile: barrier 1', 19: 'tile: panel solve', 20: 'tile: barrier 2', 21: 'tile: mfma update', 22: 'tile: stores'}
    print('tile steps', steps, '(%.1f per call)' % (steps / calls))
    for k, n in tiles.items():
        print('%-22s %8.0f cycles per step' % (n, out[k] / steps), '(owner of the diagonal tile)' if k in (16, 17, 18) else '(wave 7)' if k == 21 else '(wave 4)')
    crit = sum(out[k] for k in (16, 17, 19, 21)) / steps
    print('tile step, chain + solve + mfma: %.0f cycles per step, %.0f per pivot (the panels: 503, the finish: 219)' % (crit, crit / 16))
print('finish, whole          %8.0f cycles per call (%.0f per pivot; the panels: %.0f per pivot)' % ((out[13] + out[14]) / calls, (out[13] + out[14]) / calls / 16, out[12] / panels / 4 if panels else float('nan')))
