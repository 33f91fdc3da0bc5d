"""The grid on which the scan of the chunk sums (csrc/scan.h) runs a second round: (4097, 8194) nodes are 8197 chunks of 4096
nodes, one more than a round of 8192 chunks holds, and chunk 8192 begins at node 2 of row 8190.  The node grid of
test_gpu_quadrature_edges.py's test_chunk_scan_beyond_8192_chunks; the smallest 2-D shape of this width that gets there."""
import numpy as np

N = (4097, 8194)
CHUNK, SCAN = 4096, 8192      # nodes per chunk; chunks per round of the scan
assert -(-N[0] * N[1] // CHUNK) == SCAN + 5 and SCAN * CHUNK == 8190 * N[0] + 2


def isolated_nodes():
    """(I, J, linear index), ascending by linear index (axis 0 fastest): 90 nodes, any two at least 11 columns or 8000 rows apart
    (no two within a window of 10 nodes, none Kuhn neighbours), 45 in rows 0..18 (chunks below 20) and 45 in rows 8191..8193
    (chunks 8192..8196), the grid's first and last node and a node of the last column among them"""
    k = np.arange(42)
    cols = np.concatenate([[0], 11 + 97 * k, [N[0] - 13, N[0] - 1]])
    low = np.concatenate([[0], (5 * k) % 19, [7, 18]])
    high = np.concatenate([[8191], 8191 + k % 3, [8192, N[1] - 1]])
    I, J = np.concatenate([cols, cols]), np.concatenate([low, high])
    lin = I + N[0] * J
    o = np.argsort(lin)
    I, J, lin = I[o], J[o], lin[o]
    assert len(lin) == 90 and (np.diff(lin) > 0).all() and lin[0] == 0 and lin[-1] == N[0] * N[1] - 1
    assert (lin // CHUNK < 20).sum() == 45 and (lin // CHUNK >= SCAN).sum() == 45
    return I, J, lin
