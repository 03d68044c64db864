"""What the discrete Gaussian tests share (tests/test_gauss_host.py on the CPU, tests/test_gpu_gauss.py on the device): the seeds, the
shapes the GPU tests run -- which the host implementation is held to as well -- and their model references (tests/gauss_model.py),
computed once and left unchanged."""
import functools

import gauss_model as G
import moduli as M
import params as P
import sample_cases as K

SEED, SEED2 = K.SEED, K.SEED2
# the GPU tests' signed rows: logn 3, batch 1 is one block per row, a launch smaller than a wavefront; logn 11, batch 8 is 2048 blocks,
# eight workgroups.  tests/test_gauss_host.py shows that the large case holds every magnitude 0 .. 11 with both signs under
# (SEED, SIGNED_STREAM): pinned, the outcome is deterministic.
SIGNED_SHAPES = ((3, 1), (11, 8))
SIGNED_STREAM = 41
PREMISE_MAGNITUDES = range(12)
HOST_LOGN = (3, 6)                       # the host rows: one block per row, and one larger ring degree
SCALES = (1, 65537)
# L = 3 with a 59-bit modulus off the prime table; 65537 < 30 * 65537, so the scaled rows take hp_sample_residue's division
WIDE = [P.P40[0], M.Q59, P.P50[0]]
SMALL_Q = [P.P40[0], 65537, M.Q59]
# the distribution test: 2^20 words of the model under this seed and id
DIST_SEED, DIST_STREAM, DIST_LOGN, DIST_BATCH = K.SEED, 900, 16, 16


@functools.lru_cache(maxsize=None)
def model_signed(logn, batch, stream=SIGNED_STREAM, seed=SEED):
    out = G.sample_gauss(logn, seed, stream, batch)
    out.setflags(write=False)
    return out
