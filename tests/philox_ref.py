"""The host Philox4x32-10 of the suite, in numpy, and the counter every device user of it documents.

One copy: tests/test_lime_cpu.py holds philox4x32_10 to the Random123 known answers, tests/lime_ref.py imports it from
here, and tests/test_philox_draws_gpu.py compares every device copy (csrc/head.hip, csrc/attention.hip, csrc/physionet.hip)
with it draw by draw.  Nothing here calls the HIP library.

All users share the key (low, high word of the seed) and put the call's 64-bit offset into c0, c1 -- except dropout, whose
c0, c1 is offset + element group.  The functions ctr_* restate each user's (c0, c1, c2, c3); C3_RANGE gives, per user, the
closed range c3 can take under the limits the library enforces (tests/test_philox_cpu.py asserts they are disjoint)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(key, ctr):
    """key (k0, k1), ctr (c0, c1, c2, c3): integers or uint64 arrays holding 32-bit values (broadcast) -> four uint64 arrays"""
    k0, k1 = (np.asarray(k, dtype=np.uint64) for k in key)
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in ctr])
    m = np.uint64(MASK)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        hi0, lo0, hi1, lo1 = p0 >> s32, p0 & m, p1 >> s32, p1 & m
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(W0)) & m, (k1 + np.uint64(W1)) & m
    return c0, c1, c2, c3


def u53(a, b):
    """the 53-bit uniform of ecgmm_weighted_sample from two words"""
    return ((a >> np.uint64(5)).astype(np.float64) * 67108864.0 + (b >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0


def u01(w):
    """the 24-bit fp32 uniform on [0, 1) of dropout, the attention mask and the augmentation decisions: float32(w >> 8) * 2^-24"""
    return (np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def key(seed):
    return seed & MASK, (seed >> 32) & MASK


def split64(v):
    """(low, high) 32-bit words of a 64-bit integer or uint64 array (wrapping at 2^64 like the device's unsigned long long)"""
    v = np.asarray(v, dtype=np.uint64)
    return v & np.uint64(MASK), v >> np.uint64(32)


# ---- each user's counter, as its source documents it ------------------------------------------------------------------
def ctr_dropout(offset, g):
    """csrc/head.hip dropout_fwd_kernel: element group g = element // 4 -> (low, high of offset + g, 0, 0); word element % 4"""
    lo, hi = split64(np.uint64(offset) + np.asarray(g, dtype=np.uint64))
    return lo, hi, 0, 0


def ctr_lime(offset, n, b, f):
    """csrc/lime.hip: perturbed sample n of row b (b0 included), feature f"""
    lo, hi = split64(offset)
    b, f = np.asarray(b, dtype=np.uint64), np.asarray(f, dtype=np.uint64)
    return lo, hi, n, np.uint64(0x40000000) | (b << np.uint64(12)) | f


def ctr_noise(offset, i, g):
    """csrc/physionet.hip signal_gather_augment_kernel: row i of the call, output elements 4g .. 4g+3"""
    lo, hi = split64(offset)
    return lo, hi, i, np.uint64(0x80000000) | np.asarray(g, dtype=np.uint64)


def ctr_attention(offset, pair, x):
    """csrc/attention.hip: pair = n * heads + head, x = query * ceil(S / 4) + key // 4; word key % 4"""
    lo, hi = split64(offset)
    return lo, hi, pair, np.uint64(0xC0000000) | np.asarray(x, dtype=np.uint64)


TAG_SAMPLE, TAG_ROW_Q, TAG_ROW_R = 0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF


def ctr_tag(offset, i, tag):
    """csrc/physionet.hip: draw i of ecgmm_weighted_sample (TAG_SAMPLE), row i's decisions (TAG_ROW_R flags, TAG_ROW_Q scale / shift)"""
    lo, hi = split64(offset)
    return lo, hi, i, tag


# ---- the limits the library enforces, and the c3 range each leaves (closed intervals) ---------------------------------
MAX_L = 1 << 30         # ecgmm_signal_gather_augment refuses L > 2^30 (csrc/physionet.hip, "1 <= L <= 2^30")
MAX_S = 32768           # mha_geo / ecgmm_mha_keep_mask refuse S > 32768 under dropout (csrc/attention.hip)
MAX_D = 4096            # LIME_MAX_D, csrc/lime.hip: f takes 12 bits
MAX_ROWS = 1 << 18      # LIME_MAX_B, csrc/lime.hip: b0 + b < 2^18


def c3_ranges():
    """{user: (lowest, highest c3)} at the limits above"""
    g_max = (MAX_L + 3) // 4 - 1                                # the last noise group of the longest row
    x_max = (MAX_S - 1) * ((MAX_S + 3) // 4) + (MAX_S - 1) // 4   # last query, last key block of the longest sequence
    return {
        "dropout": (0, 0),
        "lime": (0x40000000, 0x40000000 | ((MAX_ROWS - 1) << 12) | (MAX_D - 1)),
        "noise": (0x80000000, 0x80000000 | g_max),
        "attention": (0xC0000000, 0xC0000000 | x_max),
        "weighted_sample": (TAG_SAMPLE, TAG_SAMPLE),
        "row_scale_shift": (TAG_ROW_Q, TAG_ROW_Q),
        "row_flags": (TAG_ROW_R, TAG_ROW_R),
    }
