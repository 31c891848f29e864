"""Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123)
in NumPy -- TEST INFRASTRUCTURE for csrc/rng.hip (the on-device generator of datasets.py:75-84,
183-195, 240-249 draws and model.py:225-228 latents).  Pinned by Random123's published known-answer
vectors (tests/test_rng.py).  jax.random (threefry) streams are NOT reproduced: only the
distributions are part of the reference's contract."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)


def philox4x32(counter, key, rounds=10):
    """counter: (..., 4) uint32, key: (..., 2) uint32 -> (..., 4) uint32."""
    c = np.array(counter, dtype=np.uint32, copy=True)
    k = np.array(np.broadcast_to(np.asarray(key, dtype=np.uint32), c.shape[:-1] + (2,)), dtype=np.uint32, copy=True)
    for _ in range(rounds):
        p0 = c[..., 0].astype(np.uint64) * M0
        p1 = c[..., 2].astype(np.uint64) * M1
        hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), p0.astype(np.uint32)
        hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), p1.astype(np.uint32)
        c = np.stack([hi1 ^ c[..., 1] ^ k[..., 0], lo1, hi0 ^ c[..., 3] ^ k[..., 1], lo0], axis=-1)
        k = np.stack([k[..., 0] + W0, k[..., 1] + W1], axis=-1)
    return c


def normals_from_bits(bits):
    """The kernel's Box-Muller: per Philox block (4 words) two pairs; u1 = ((w >> 8) + 0.5) 2^-24 in
    (0,1), u2 = w 2^-32; (r cos t, r sin t) with r = sqrt(-2 ln u1), t = 2 pi u2.  float64 here."""
    b = np.asarray(bits, dtype=np.uint32)
    u1 = ((b[..., 0::2] >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    u2 = b[..., 1::2].astype(np.float64) * 2.0 ** -32
    r = np.sqrt(-2.0 * np.log(u1))
    out = np.empty(b.shape, dtype=np.float64)
    out[..., 0::2] = r * np.cos(2 * np.pi * u2)
    out[..., 1::2] = r * np.sin(2 * np.pi * u2)
    return out


U1_MAX = np.float32(1.0 - 2.0 ** -24)          # 0x1.fffffep-1f: the largest float32 below 1, normals4's clamp on u1


def kernel_uniforms(bits):
    """The float32 uniforms rng_dev.h's normals4 forms, bit for bit (NumPy float32 rounds as the device does): per pair
    u1 = min(((float)(w >> 8) + 0.5f) 2^-24, 0x1.fffffep-1f) -- from w >> 8 = 2^23 on the sum is a tie and rounds to even, down
    or up by a half, for w >> 8 = 2^24 - 1 to 2^24, which the clamp takes back below 1 -- and u2 = (float)w 2^-32, which rounds too and may be 1."""
    b = np.asarray(bits, dtype=np.uint32)
    u1 = ((b[..., 0::2] >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    u2 = b[..., 1::2].astype(np.float32) * np.float32(2.0 ** -32)
    return np.minimum(u1, U1_MAX), u2


def normals_kernel_uniform(bits):
    """The KERNEL-UNIFORM reference: Box-Muller in float64 on the kernel's own float32 uniforms (kernel_uniforms).  What is left
    between it and the device is the device's float32 transcendentals and products alone; normals_from_bits is the ideal
    reference, from which both differ by design wherever u1 was rounded."""
    u1, u2 = (u.astype(np.float64) for u in kernel_uniforms(bits))
    r = np.sqrt(-2.0 * np.log(u1))
    out = np.empty(np.asarray(bits).shape, dtype=np.float64)
    out[..., 0::2] = r * np.cos(2 * np.pi * u2)
    out[..., 1::2] = r * np.sin(2 * np.pi * u2)
    return out


def stream_bits(seed, step, tag, row0, rows, q0, nblk):
    """Philox words [rows, nblk, 4] of blocks q0 .. q0 + nblk - 1 of rows row0 .. row0 + rows - 1, the counter rule of
    sample_normals: counter = ((row0 + i) mod 2^32, q, step, tag), key = (seed_lo, seed_hi)."""
    ctr = np.empty((rows, nblk, 4), dtype=np.uint32)
    ctr[..., 0] = ((int(row0) + np.arange(rows, dtype=np.int64)) & 0xFFFFFFFF).astype(np.uint32)[:, None]
    ctr[..., 1] = (q0 + np.arange(nblk)).astype(np.uint32)[None, :]
    ctr[..., 2] = np.uint32(int(step) & 0xFFFFFFFF)
    ctr[..., 3] = np.uint32(int(tag) & 0xFFFFFFFF)
    key = np.array([int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    return philox4x32(ctr, key)


def batch_reference(kind, A, dd, did, pad, var, rows, row0, seed, step, tag, L, D, normals=normals_kernel_uniform):
    """A whole vaek_make_batch batch in float64: (x [rows, D], z1 [rows, L], z2 [rows, D], deps).  kind 0 linear_gaussian
    (x = [A n, 0 ...] + sqrt(var) nu, A [dd, did]), 1 sigmoid ([n, sigmoid(n . a), 0 ...]), 2 sphere ([n / |n|, 0 ...]).  The
    dataset normals n are the first did (kind 0) or dd of the row's stream under `tag`, the noise normals nu (var > 0) its blocks
    from noise_block_offset(did) on, the latents [z1 | z2] the first L + D of the stream under tag + 2^30.  `normals` maps Philox
    words to normals (the kernel-uniform reference by default).  deps: the reference normals every element of x was formed from,
    {"n": [rows, nn], "nu": [rows, D] or None}, for per-element error bounds."""
    assert D == dd + pad + (1 if kind == 1 else 0)
    nn = did if kind == 0 else dd

    def draw(tag_, q0, count):
        nblk = (count + 3) // 4
        return normals(stream_bits(seed, step, tag_, row0, rows, q0, nblk)).reshape(rows, 4 * nblk)[:, :count]
    n = draw(tag, 0, nn)
    nu = None
    x = np.zeros((rows, D))
    if kind == 0:
        x[:, :dd] = n @ np.asarray(A, np.float64).reshape(dd, did).T
        if var > 0:
            nu = draw(tag, noise_block_offset(did), D)
            x += np.sqrt(float(var)) * nu
    elif kind == 1:
        x[:, :dd] = n
        x[:, dd] = 1.0 / (1.0 + np.exp(-(n @ np.asarray(A, np.float64).reshape(dd))))
    else:
        x[:, :dd] = n / np.linalg.norm(n, axis=1, keepdims=True)
    z = draw((int(tag) + 0x40000000) & 0xFFFFFFFF, 0, L + D)
    return x, z[:, :L].copy(), z[:, L:].copy(), {"n": n, "nu": nu}


def sample_normals(seed, step, tag, sample_index, n):
    """n normals of one sample row exactly as csrc/rng.hip draws them: block q uses
    counter = (sample_lo, q, step, tag), key = (seed_lo, seed_hi)."""
    nblk = (n + 3) // 4
    ctr = np.zeros((nblk, 4), dtype=np.uint32)
    ctr[:, 0] = np.uint32(sample_index & 0xFFFFFFFF)
    ctr[:, 1] = np.arange(nblk, dtype=np.uint32)
    ctr[:, 2] = np.uint32(step & 0xFFFFFFFF)
    ctr[:, 3] = np.uint32(tag)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    return normals_from_bits(philox4x32(ctr, key)).reshape(-1)[:n]


def noise_block_offset(did):
    """Dataset noise normals (linear_gaussian var_added > 0) start at Philox block ceil(did / 4) of the row's
    dataset stream, one block per 4 data dims -- exactly as csrc/rng.hip draws them."""
    return (did + 3) // 4
