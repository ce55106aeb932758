"""A host replica of the device noise (csrc/common.h: Philox4x32-10) and of every map from a launch's elements to its draws.  numpy
only, vectorised; nothing here touches the GPU or torch.  tests/test_philox_ref.py anchors the generator (published vectors, the
project's own header compiled for the host); tests/test_gpu_device_noise.py runs every kernel once on its own draws and once on the
tensors built here and asks for equal bits.

One draw is Philox::gen(seed, stream, counter): counter words {counter_lo, counter_hi, stream_lo, stream_hi}, key {seed_lo, seed_hi},
ten rounds, the key bumped by the Weyl constants 0x9E3779B9 / 0xBB67AE85 after each.  It gives four 32-bit lanes;
u01(bits) = (bits >> 8) * 2^-24 is exact in float32, so the device's uniform and the replica's are the same float32 or a bug.

The maps, as read from the kernels.  Element (row r, entry v) of a launch gets (stream, counter, lane):

  roll-out / sampler step t          stream t, counter (r V + v) >> 2, lane (r V + v) & 3                       rollout_u
    csrc/decoder.hip    gumbel_softmax_argmax_kernel      any V: idx = r V + v, gen(idx >> 2)[idx & 3]
    csrc/decoder.hip    gumbel_softmax_argmax_reg_kernel  V % 4 == 0: counter r (V >> 2) + q, lanes = entries 4 q .. 4 q + 3
    csrc/decoder_step.hip  vocab_step                     V % 4 == 0: counter r (V >> 2) + (v >> 2)
    csrc/gemm.hip       EPI_GUMBELMAX (tile8)             V % 4 == 0, operands swapped (M = V, n = r): counter n (M >> 2) + (m0 >> 2)
    csrc/attn_rollout.hip                                 the same kernels, stream t
  teacher-forced decode with noise   stream 0x7466, row r = b Tmax + t, the roll-out's map over [B Tmax, V]      tf_u
    csrc/teacher_forced.hip -> gumbel_softmax_argmax_kernel
  top-k / nucleus draw               stream t (sample_captions) or the caller's stream_id (sample_logits),      sample_u
    csrc/sample.hip     sample_select                     counter r ceil(V / 4) + (v >> 2), lane v & 3: rows never share a
                                                          counter, so for V % 4 != 0 this is NOT the roll-out's map
  scheduled sampling, step t >= 1    coin:  stream "ssco" << 32 | t, counter b, lane 0                           ss_coin
    csrc/sched_sample.hip ss_pick_kernel                  noise: stream "ssno" << 32 | t, counter b << 32 | (v >> 2), lane v & 3   ss_noise
                                                          (the vector form, V % 4 == 0, and the scalar form index alike)
  highway dropout                    stream 0x44495343 ("DISC"), counter (m >> 2) N + n, lane m & 3, keep = u >= p           highway_keep
    csrc/gemm_device.h  highway_keep4                     N is F, the UNPADDED feature count, at all three callers: gemm_kernel's scalar
                                                          highway epilogue and tile8's wide one (disc_highway_fwd sets g.N = c.F; Fp is
                                                          only the leading dimension) and disc_highway_redrop_kernel (passes F).

Stream tags: roll-out streams are the step index t < L; 0x7466 would be step 29798 of a roll-out, and the library takes L <= 1024
(the trainers L <= 64): unreachable.  The other tags are far above every step index and differ among themselves."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32, MASK64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF

STREAM_TF = 0x7466
STREAM_DISC = 0x44495343
STREAM_SS_COIN = 0x7373636F << 32      # "ssco"
STREAM_SS_NOISE = 0x73736E6F << 32     # "ssno"


def _u64(x):
    """Python ints (any value mod 2^64) or integer arrays -> uint64 array."""
    if isinstance(x, (int, np.integer)):
        return np.array(int(x) & MASK64, dtype=np.uint64)
    x = np.asarray(x)
    if x.dtype == object:
        return np.array([int(v) & MASK64 for v in x.reshape(-1)], dtype=np.uint64).reshape(x.shape)
    return x.astype(np.uint64)


def philox4x32_10(seed, stream, counter):
    """uint32[..., 4]: Philox::gen(seed, stream, counter) of csrc/common.h, broadcast over the three arguments."""
    seed, stream, counter = np.broadcast_arrays(_u64(seed), _u64(stream), _u64(counter))
    lo, s32 = np.uint64(MASK32), np.uint64(32)
    c0, c1, c2, c3 = counter & lo, counter >> s32, stream & lo, stream >> s32
    k0, k1 = seed & lo, seed >> s32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2           # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & lo, (p0 >> s32) ^ c3 ^ k1, p0 & lo
        k0, k1 = (k0 + np.uint64(W0)) & lo, (k1 + np.uint64(W1)) & lo
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def u01(bits):
    """Philox::u01: the top 24 bits as a float32 in [0, 1 - 2^-24]."""
    return (np.asarray(bits, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def _draw(seed, stream, counter, lane):
    """u01 of lane `lane` of the draw at `counter` (arrays of one shape)."""
    bits = philox4x32_10(seed, stream, counter)
    return u01(np.take_along_axis(bits, np.asarray(lane, dtype=np.int64)[..., None], -1)[..., 0])


# ---------------------------------------------------------------------------------------------------------------- the maps
# Each *_triples function IS the map written down: (stream, counter, lane) as uint64 / uint64 / int64 arrays of the tensor's shape
# (from_triples turns them into the tensor, one Philox call per element).  Each *_u / *_keep function builds the same tensor with one
# call per COUNTER, four elements at a time -- what the big shapes need; tests/test_philox_ref.py holds the two forms equal.
def from_triples(seed, triples):
    return _draw(seed, *triples)


def _lanes(seed, stream, counters):
    """float32 [..., 4]: the four uniforms of each counter."""
    return u01(philox4x32_10(seed, stream, counters))


def rollout_triples(t, rows, V):
    idx = (np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(V) + np.arange(V, dtype=np.uint64)[None, :])
    return np.full(idx.shape, int(t), dtype=np.uint64), idx >> np.uint64(2), (idx & np.uint64(3)).astype(np.int64)


def rollout_u(seed, t, rows, V):
    """float32 [rows, V]: the uniforms of roll-out step t (the flat element index r V + v, four per counter, across row ends)."""
    n = rows * V
    return _lanes(seed, int(t), np.arange((n + 3) // 4, dtype=np.uint64)).reshape(-1)[:n].reshape(rows, V)


def rollout_us(seed, L, rows, V):
    """float32 [L, rows, V]: noise_u of a roll-out of L steps."""
    return np.stack([rollout_u(seed, t, rows, V) for t in range(L)])


def tf_triples(B, Tmax, V):
    s, c, l = rollout_triples(STREAM_TF, B * Tmax, V)
    return s.reshape(B, Tmax, V), c.reshape(B, Tmax, V), l.reshape(B, Tmax, V)


def tf_u(seed, B, Tmax, V):
    """float32 [B, Tmax, V]: noise_u of a teacher-forced decode with pretrain = 0 (row b Tmax + t of ONE launch over all steps)."""
    return rollout_u(seed, STREAM_TF, B * Tmax, V).reshape(B, Tmax, V)


def sample_triples(stream, rows, V):
    nq = (V + 3) // 4
    v = np.arange(V, dtype=np.uint64)[None, :]
    ctr = np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(nq) + (v >> np.uint64(2))
    return np.full(ctr.shape, int(stream) & MASK64, dtype=np.uint64), ctr, np.broadcast_to((v & np.uint64(3)).astype(np.int64), ctr.shape)


def sample_u(seed, stream, rows, V):
    """float32 [rows, V]: the uniforms of one top-k / nucleus draw (stream = the step t or sample_logits' stream_id)."""
    nq = (V + 3) // 4
    return _lanes(seed, int(stream) & MASK64, np.arange(rows * nq, dtype=np.uint64)).reshape(rows, 4 * nq)[:, :V].copy()


def sample_us(seed, L, rows, V):
    """float32 [L, rows, V]: noise_u of sample_captions."""
    return np.stack([sample_u(seed, t, rows, V) for t in range(L)])


def ss_coin_triples(t, B):
    b = np.arange(B, dtype=np.uint64)
    return np.full(B, STREAM_SS_COIN | int(t), dtype=np.uint64), b, np.zeros(B, dtype=np.int64)


def ss_coin(seed, B, Lc):
    """float32 [B, Lc]: coin_u of a scheduled-sampling decode; column t - 1 is step t's coin (t = 1 .. Lc)."""
    return np.stack([_lanes(seed, STREAM_SS_COIN | t, np.arange(B, dtype=np.uint64))[:, 0] for t in range(1, Lc + 1)], 1)


def ss_noise_triples(t, B, V):
    v = np.arange(V, dtype=np.uint64)[None, :]
    ctr = (np.arange(B, dtype=np.uint64)[:, None] << np.uint64(32)) | (v >> np.uint64(2))
    return np.full(ctr.shape, STREAM_SS_NOISE | int(t), dtype=np.uint64), ctr, np.broadcast_to((v & np.uint64(3)).astype(np.int64), ctr.shape)


def ss_noise(seed, B, Lc, V):
    """float32 [Lc, B, V]: noise_u of a scheduled-sampling decode; slice t - 1 is step t's (t = 1 .. Lc)."""
    nq = (V + 3) // 4
    ctr = (np.arange(B, dtype=np.uint64)[:, None] << np.uint64(32)) | np.arange(nq, dtype=np.uint64)[None, :]
    return np.stack([_lanes(seed, STREAM_SS_NOISE | t, ctr).reshape(B, 4 * nq)[:, :V] for t in range(1, Lc + 1)])


def highway_triples(M, N):
    m = np.arange(M, dtype=np.uint64)[:, None]
    ctr = (m >> np.uint64(2)) * np.uint64(N) + np.arange(N, dtype=np.uint64)[None, :]
    return np.full(ctr.shape, STREAM_DISC, dtype=np.uint64), ctr, np.broadcast_to((m & np.uint64(3)).astype(np.int64), ctr.shape)


def highway_u(seed, M, N):
    """float32 [M, N]: the uniform behind each keep flag (one counter per 4 rows x 1 column)."""
    nq = (M + 3) // 4
    u = _lanes(seed, STREAM_DISC, np.arange(nq * N, dtype=np.uint64)).reshape(nq, N, 4)
    return u.transpose(0, 2, 1).reshape(4 * nq, N)[:M].copy()


def highway_keep(seed, M, N, drop_p):
    """uint8 [M, N]: the keep mask of the highway dropout over M rows and N = F features: keep = u >= p, compared in float32."""
    return (highway_u(seed, M, N) >= np.float32(drop_p)).astype(np.uint8)
