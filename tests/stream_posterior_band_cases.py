"""Shared by tests/test_stream_posterior_band_cpu.py and tests/test_stream_posterior_band_gpu.py: the names of the band route's
C entry points, banded problems in both forms of the input (log scores and probabilities) with the band a caller would state
for them, and the tile sizes of the band kernels for 256 compute units.

Everything else -- `Feeder`, `ragged_plan`, `reference`, the bounds -- is tests/stream_posterior_cases.py's, and the matrices
are tests/stream_band_cases.py's `band_matrix`."""
import math

import numpy as np
import torch

from stream_band_cases import band_matrix
from stream_posterior_cases import problem

NAMES = ('torbi_hip_stream_smooth_band_covers', 'torbi_hip_stream_smooth_band_tile', 'torbi_hip_stream_smooth_band_diagonals_size',
         'torbi_hip_stream_smooth_band_prepare', 'torbi_hip_stream_smooth_band_push', 'torbi_hip_stream_smooth_band_flush')
EINVAL, EWORKSPACE, ERANGE, EUNSUPPORTED = -1, -2, -3, -5
MAX_STATES = 4096                       # include/torbi_hip.h: _covers answers 0 above
MAX_WINDOW = 64                         # min(reach_left + reach_right + 1, S) at most
BACKGROUNDS = (-math.inf, -20., -3.)
TINY = float(np.log(np.float32(np.finfo(np.float32).tiny)))

# (G, the smallest batch that gets it) at few states and a narrow band, for 256 compute units: 8 streams per workgroup, halved
# while there are fewer workgroups than compute units
TILES = ((1, 1), (2, 511), (4, 1021), (8, 2041))


def lds_bytes(G, S, reach_left, reach_right):
    """LDS of a tile of G streams: the rows [2][G][S + 2 halo] and the wave sums [2][G][16], fp32."""
    halo = max(min(reach_left, S - 1), min(reach_right, S - 1))
    return 2 * G * (S + 2 * halo + 16) * 4


def band_problem(B, T, S, reach_left, reach_right, background, log_probs, seed):
    """(observation (B, T, S), transition (S, S), initial (S,), band): what a caller hands StreamPosteriors in the form
    `log_probs` says, and the band=(reach_left, reach_right, background) that is true of the matrix after the preparation.
    In probabilities the background is what torch.log makes of the one probability outside the band."""
    obs, _, init = problem(B, T, S, 'none', log_probs, seed)
    scores = torch.from_numpy(band_matrix(S, reach_left, reach_right, background, seed=seed))
    if log_probs:
        return obs, scores, init, (reach_left, reach_right, float(background))
    trans = torch.exp(scores)
    j, i = np.meshgrid(np.arange(S), np.arange(S), indexing='ij')
    outside = torch.log(trans).numpy()[(i < j - reach_left) | (i > j + reach_right)]
    if outside.size:
        assert (outside.view(np.uint32) == outside.view(np.uint32)[0]).all()       # one value, bit for bit
        background = float(outside[0])
    return obs, trans, init, (reach_left, reach_right, float(background))


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)
