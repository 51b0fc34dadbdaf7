"""The draw contract of ``include/cough_amd_draws.h`` restated in numpy (``cough_detector_amd/draws.py``, ``csrc/draws.hip``).

Philox4x32-10 runs in ``uint64`` arithmetic masked to 32 bits; every draw is float64 arithmetic, one IEEE operation per
operator (numpy has no fused multiply-add), conversions to int truncate toward zero.  ``draw_ref`` returns the records
as arrays, field by field, and the mask triples as int32 ``(3, B, n_masks)``; the GPU test compares them bit for bit
with what ``cough_draw_batch`` wrote.
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
CLIP_DTYPE = np.dtype([("shift", "<i4"), ("gain", "<f4"), ("gaussian", "<i4"), ("bank_index", "<i4"),
                       ("gaussian_snr_db", "<f8"), ("bank_snr_db", "<f8"), ("bank_start", "<i8")])   # cough_aug_clip, 40 bytes


def philox4x32_10(counter, key):
    """counter: four arrays (or scalars) of 32-bit words, key: (lo, hi) -> four uint64 arrays holding 32-bit words."""
    c = [np.asarray(v, dtype=np.uint64) & M32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint64(key[0]) & M32, np.uint64(key[1]) & M32
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                                  # < 2^64: both factors are < 2^32
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & M32, p1 >> np.uint64(32), p1 & M32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def unit(x):
    """u = (x + 0.5) * 2^-32 in float64: exact, strictly inside (0, 1)."""
    return (np.asarray(x, dtype=np.uint64).astype(np.float64) + 0.5) * 2.0 ** -32


def slot(seed, s, rows):
    """The four uniforms of Philox block (s, row, 0, 1) under ``seed`` for every row."""
    seed = int(seed) & (2**64 - 1)
    words = philox4x32_10((np.full(rows.shape, s, dtype=np.uint64), rows, 0, 1), (seed & 0xFFFFFFFF, seed >> 32))
    return [unit(w) for w in words]


def repeated_length(bl, n):
    return np.where(bl < n, (n // np.maximum(bl, 1) + 1) * bl, bl)


def draw_ref(seed, lengths, p_augment, bank_lengths, spec_p, n_freq_masks, freq_mask_param, n_time_masks,
             time_mask_param, height, width):
    """-> (clips: structured array of CLIP_DTYPE or None when p_augment is None, masks: int32 (3, B, n_masks) or None when
    spec_p is None or there is no mask, fired: dict of the boolean coins)."""
    n = np.asarray(lengths, dtype=np.int64)
    b = n.size
    rows = np.arange(b, dtype=np.uint64)
    s2 = slot(seed, 2, rows)
    clips = masks = None
    fired = {}
    if p_augment is not None:
        s0, s1 = slot(seed, 0, rows), slot(seed, 1, rows)
        clips = np.zeros(b, dtype=CLIP_DTYPE)
        clips["gain"], clips["bank_index"] = 1.0, -1
        f_shift, f_gain, f_gauss = s0[0] <= p_augment, s0[2] <= p_augment, s1[0] <= p_augment
        shift = (n.astype(np.float64) * (-0.2 + 0.4 * s0[1])).astype(np.int32)         # astype truncates toward zero
        clips["shift"] = np.where(f_shift, shift, 0)
        clips["gain"] = np.where(f_gain, (0.7 + 0.6 * s0[3]).astype(np.float32), np.float32(1.0))
        clips["gaussian"] = f_gauss
        clips["gaussian_snr_db"] = np.where(f_gauss, 10.0 + 20.0 * s1[1], 0.0)
        bl_all = np.asarray(bank_lengths, dtype=np.int64)
        n_bank = bl_all.size
        f_bank = (s1[2] <= p_augment) & (n_bank > 0)
        if n_bank > 0:
            k = np.minimum((s2[0] * float(n_bank)).astype(np.int32), n_bank - 1)
            rep = repeated_length(bl_all[k], n)
            start = np.minimum((s2[1] * (rep - n + 1).astype(np.float64)).astype(np.int64), rep - n)
            clips["bank_index"] = np.where(f_bank, k, -1)
            clips["bank_start"] = np.where(f_bank, start, 0)
            clips["bank_snr_db"] = np.where(f_bank, 5.0 + 15.0 * s1[3], 0.0)
        fired.update(shift=f_shift, gain=f_gain, gaussian=f_gauss, bank=f_bank)
    n_masks = n_freq_masks + n_time_masks
    if spec_p is not None and n_masks > 0:
        f_spec = s2[3] <= spec_p
        masks = np.zeros((3, b, n_masks), dtype=np.int32)
        for m in range(n_masks):
            axis = 0 if m < n_freq_masks else 1
            param, size = (freq_mask_param, height) if axis == 0 else (time_mask_param, width)
            s = slot(seed, 3 + m, rows)
            value = s[0] * float(param)
            minv = s[1] * (float(size) - value)
            start = minv.astype(np.int32)
            end = start + value.astype(np.int32)
            masks[0, :, m] = np.where(f_spec, axis, 0)
            masks[1, :, m] = np.where(f_spec, start, 0)
            masks[2, :, m] = np.where(f_spec, end, 0)
        fired.update(spec=f_spec)
    return clips, masks, fired
