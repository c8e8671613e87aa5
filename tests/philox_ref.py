"""A numpy replica of gmr::Philox::gen(seed, subseq, offset) (csrc/gmr_common.h: Philox-4x32-10, counter
(offset lo, offset hi, subseq lo, subseq hi), key (seed lo, seed hi) bumped after every round), vectorised over
offsets, with u32_to_unit and the site mixing of csrc/rf.hip.  Pinned to the kernels bit for bit through
gmr_frd_prune_keys (tests/test_frd_select_shapes_gpu.py) and gmr_rf_rand (tests/test_rf_kernels_shapes_gpu.py)."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
SITE_MIX = 0x9E3779B97F4A7C15
FRD_KEY_MIX = 0xF2EED0F2EED0  # frd_keys_kernel: seed ^ this
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox(seed, subseq, offsets):
    """The four uint32 words of every offset: (len(offsets), 4)."""
    off = np.asarray(offsets, dtype=np.uint64)
    seed, subseq = int(seed) & (2 ** 64 - 1), int(subseq) & (2 ** 64 - 1)
    c = [off & LO, off >> S32, np.full_like(off, subseq & 0xFFFFFFFF), np.full_like(off, subseq >> 32)]
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 -> 64 bits, no overflow
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & LO, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & LO]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=1).astype(np.uint32)


def site_seed(seed, site):
    """seed + site * SITE_MIX (mod 2^64): the key of the rf.hip draws at one site."""
    return (int(seed) + int(site) * SITE_MIX) & (2 ** 64 - 1)


def u32_to_unit(x):
    """gmr::u32_to_unit: ((x >> 8) + 1) / 2^24 in (0, 1], exact in fp32."""
    hi24 = (np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)
    return (hi24 + np.float32(1)) * np.float32(2.0 ** -24)
