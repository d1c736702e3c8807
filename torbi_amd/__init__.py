"""torbi_amd -- MI355X-native batched Viterbi decoding behind torbi's API.

Drop-in for ONE path of maxrmorrison/torbi: from_probabilities / from_file* -> decode ->
viterbi_decode (reference torbi/core.py:110-368, torbi/viterbi.py:5-53,
torbi/csrc/ops.cpp:17), computed by hand-written gfx950 HIP kernels reached through the C
ABI in include/torbi_hip.h.  `gpu=None` selects, like upstream, the CPU operator: its twin behind
include/torbi_cpu.h (`decode_cpu`), an explicit entry point -- the HIP path has no CPU fallback.
"""
from .viterbi import decode, decode_batches, decode_cpu, decode_uniform, workspace_bytes, set_forward_path, forward_path
from .core import (BATCH_SIZE, NUM_WORKERS, from_probabilities, from_file, from_file_to_file,
                   from_files_to_files, from_dataloader, save, save_masked)
from . import data
from .chunk import chunk
from . import synth
from . import distributed
from . import margins
from . import paths
from . import entropy
from . import timer
from .pipeline import DecodePipeline
from .state import reset as reset_path_state
from .core import release_job_memory
from .stream import StreamDecoder, stream_route
from .stream_posterior import StreamPosteriors, stream_posterior_route
from .posterior import (forward_backward, forward_backward_banded, forward_backward_banded_workspace_bytes,
                        forward_backward_workspace_bytes, posterior_route, state_posteriors)
from .training import (band_counts_to_dense, counts_route, expected_counts, expected_counts_banded_workspace_bytes,
                       expected_counts_workspace_bytes, forward_backward_counts, forward_backward_counts_banded,
                       log_likelihood)
from .k_best import (best_paths, decode_k_best, decode_k_best_banded, decode_k_best_banded_workspace_bytes,
                     decode_k_best_workspace_bytes, k_best_route)
from .sampling import (forward_sample, forward_sample_banded, forward_sample_banded_workspace_bytes,
                       forward_sample_workspace_bytes, sample_paths, sample_route)

__all__ = ['decode', 'decode_batches', 'decode_cpu', 'chunk', 'decode_uniform', 'workspace_bytes', 'set_forward_path', 'forward_path', 'from_probabilities', 'from_file', 'from_file_to_file',
           'from_files_to_files', 'from_dataloader', 'save', 'save_masked', 'data', 'synth',
           'distributed', 'DecodePipeline', 'BATCH_SIZE', 'NUM_WORKERS', 'reset_path_state', 'release_job_memory', 'timer',
           'StreamDecoder', 'state_posteriors', 'forward_backward', 'forward_backward_workspace_bytes',
           'expected_counts', 'expected_counts_workspace_bytes', 'forward_backward_counts', 'log_likelihood',
           'best_paths', 'decode_k_best', 'decode_k_best_workspace_bytes', 'forward_backward_banded',
           'forward_backward_banded_workspace_bytes', 'posterior_route', 'forward_backward_counts_banded',
           'expected_counts_banded_workspace_bytes', 'band_counts_to_dense', 'counts_route', 'stream_route', 'decode_k_best_banded',
           'decode_k_best_banded_workspace_bytes', 'k_best_route', 'sample_paths', 'forward_sample',
           'forward_sample_workspace_bytes', 'forward_sample_banded', 'forward_sample_banded_workspace_bytes', 'sample_route',
           'StreamPosteriors', 'stream_posterior_route', 'margins', 'paths', 'entropy']
