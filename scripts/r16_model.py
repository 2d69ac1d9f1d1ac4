#!/usr/bin/env python
"""Lane-level numpy model of csrc/rank16_mfma.hip's fragment index arithmetic (v_mfma_f32_16x16x32 operand layouts of
csrc/mfma16.hpp, ds_read_b64_tr_b16 as verified on hardware by tests/test_gpu_parity_r4.py::test_ds_read_tr16_b64_semantics):
rank_update16's interleaved transposed product and bwd_g16's two phases must reproduce plain matrix products."""
import numpy as np

L = np.arange(64)
ROW, KQ = L & 15, L >> 4


def mfma(a, b, c=None):
    """a[lane][e]: A[row = lane & 15][k = 8 (lane >> 4) + e]; b[lane][e]: B[k][col = lane & 15]; returns d[lane][reg] =
    D[row = 4 (lane >> 4) + reg][col = lane & 15]."""
    A = np.zeros((16, 32)); B = np.zeros((32, 16))
    for l in range(64):
        for e in range(8):
            A[l & 15, 8 * (l >> 4) + e] = a[l][e]
            B[8 * (l >> 4) + e, l & 15] = b[l][e]
    D = A @ B
    d = np.zeros((64, 4))
    for l in range(64):
        for reg in range(4):
            d[l][reg] = D[4 * (l >> 4) + reg, l & 15]
    return d if c is None else c + d


def rank_update16(T, U):
    """one 16-row slab x one 32-column group: out[m, n] = sum_j T[m, j] U[n, j]"""
    r = T.shape[1]
    out = np.zeros((16, 32))
    th = np.zeros((64, 8))
    for l in range(64):
        mm, q = l & 15, l >> 4
        for e in range(8):
            j = 8 * (q & 1) + e
            th[l][e] = T[mm, j] if j < r else 0.0
    d = []
    for tile in range(2):
        ua = np.zeros((64, 8))
        for l in range(64):
            mm, q = l & 15, l >> 4
            n = 8 * (mm >> 2) + 4 * tile + (mm & 3)
            for e in range(8):
                j = 8 * (q & 1) + e
                ua[l][e] = (U[n, j] if j < r else 0.0) if q < 2 else 0.0   # hi part only (lo = 0 in exact arithmetic)
        d.append(mfma(ua, th))
    for l in range(64):
        mm, q = l & 15, l >> 4
        for reg in range(4):
            out[mm, 8 * q + reg] = d[0][l][reg]
            out[mm, 8 * q + 4 + reg] = d[1][l][reg]
    return out


def tr_read(stage, pitch, q, i, row_off, c0):
    """lane (q, i): supplies the address of row 4 q + i / 4, columns c0 + 4 (i % 4); receives rows 4 q .. 4 q + 3 of column
    c0 + i of the 16-row block starting at row_off"""
    return [stage[row_off + 4 * q + e, c0 + i] for e in range(4)]


def bwd_g16_unit(G, T, U):
    """one 32-row x 32-column unit: Gt partial [32, 16] = G U, dUp partial [32 cols, 16] = G^T T"""
    r = T.shape[1]
    # phase 1
    uh = np.zeros((64, 8))
    for l in range(64):
        jj, kq = l & 15, l >> 4
        for e in range(8):
            uh[l][e] = U[8 * kq + e, jj] if jj < r else 0.0
    gt = np.zeros((32, 16))
    for rg in range(2):
        cur = np.zeros((64, 8))
        for l in range(64):
            jj, q = l & 15, l >> 4
            cur[l] = G[rg * 16 + jj, 8 * q:8 * q + 8]
        d1 = mfma(cur, uh)
        for l in range(64):
            jj, q = l & 15, l >> 4
            for reg in range(4):
                gt[rg * 16 + 4 * q + reg, jj] = d1[l][reg]
    # phase 2: the stage tile is the unit itself (row jj / 16 + jj, columns 8 q ..)
    stage = G.copy()
    tf = np.zeros((64, 8))
    for l in range(64):
        jj, q = l & 15, l >> 4
        for e in range(8):
            row = 4 * q + e if e < 4 else 16 + 4 * q + (e - 4)
            tf[l][e] = T[row, jj] if jj < r else 0.0
    dup = np.zeros((32, 16))
    for nt in range(2):
        a = np.zeros((64, 8))
        for l in range(64):
            jj, q = l & 15, l >> 4
            a[l][:4] = tr_read(stage, None, q, jj, 0, 16 * nt)
            a[l][4:] = tr_read(stage, None, q, jj, 16, 16 * nt)
        d2 = mfma(a, tf)
        for l in range(64):
            jj, q = l & 15, l >> 4
            for reg in range(4):
                dup[16 * nt + 4 * q + reg, jj] = d2[l][reg]
    return gt, dup


def rowdot16_step(X, F):
    """one 16-row slab x one 32-column k-step: T[m, j] = sum_c X[m, c] F[j, c]"""
    r = F.shape[0]
    fh, cur = np.zeros((64, 8)), np.zeros((64, 8))
    for l in range(64):
        jj, kq = l & 15, l >> 4
        cur[l] = X[jj, 8 * kq:8 * kq + 8]
        if jj < r:
            fh[l] = F[jj, 8 * kq:8 * kq + 8]
    d = mfma(cur, fh)
    t = np.zeros((16, 16))
    for l in range(64):
        jj, q = l & 15, l >> 4
        for reg in range(4):
            t[4 * q + reg, jj] = d[l][reg]
    return t


PITCH = 96  # kR16Pitch: bytes per row of a wave's 32 x 32 16-bit staging tile


def bf16_round(v):
    """nearest-even bfloat16 of float32 values, as float64 (E::from_f of csrc/common.hpp for finite values)"""
    u = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def split_hi_lo(v):
    """mfma16.hpp's split_hi_lo: v ~ hi + lo, both bf16"""
    v32 = np.asarray(v, np.float32)
    hi = bf16_round(v32)
    lo = bf16_round((v32.astype(np.float64) - hi).astype(np.float32))
    return hi, lo


def colreduce16_step(X, T, sl, split=False):
    """colreduce16_mfma_kernel, one wave, one 32-row step of one 32-column group, slice `sl`: the two 16-byte pieces per lane
    go to the wave's staging tile (byte addresses at PITCH), come back column-major through the two transpose reads, and
    meet the step's T fragment (lane jj <-> rank 16 sl + jj, zero at or past r; k slot 8 q + e <-> row 4 q + e / 16 + 4 q +
    e - 4).  X: [rows <= 32, 32] (bf16-exact values), T: [rows, r].  Returns acc[nt][lane][reg]; split: T enters as
    hi + lo into the same accumulator."""
    rows, r = T.shape
    stage = np.zeros(32 * PITCH // 2)   # the tile in 16-bit elements
    for l in range(64):
        jj, q = l & 15, l >> 4
        for rg in range(2):
            row = rg * 16 + jj
            piece = X[row, 8 * q:8 * q + 8] if row < rows else np.zeros(8)
            a0 = (row * PITCH + q * 16) // 2
            stage[a0:a0 + 8] = piece
    tile = np.zeros((32, 32))
    for row in range(32):
        tile[row] = stage[row * PITCH // 2:row * PITCH // 2 + 32]
    tf = np.zeros((64, 8))
    for l in range(64):
        jj, q = l & 15, l >> 4
        j = 16 * sl + jj
        for e in range(8):
            row = 4 * q + e if e < 4 else 16 + 4 * q + (e - 4)
            tf[l][e] = T[row, j] if (row < rows and j < r) else 0.0
    frags = split_hi_lo(tf) if split else (tf,)
    acc = []
    for nt in range(2):
        a = np.zeros((64, 8))
        for l in range(64):
            jj, q = l & 15, l >> 4
            a[l][:4] = tr_read(tile, PITCH, q, jj, 0, 16 * nt)
            a[l][4:] = tr_read(tile, PITCH, q, jj, 16, 16 * nt)
        d = np.zeros((64, 4))
        for f in frags:
            d = mfma(a, f, d)
        acc.append(d)
    return acc


def colreduce16(X, T, layout="RK", split=False):
    """D = T^T X for X [M, K] (K % 32 == 0), T [M, r], 9 <= r <= 64, as the kernel's waves walk it: NS = ceil(r / 16) slices,
    32-row steps (the last one ragged), one wave per 32-column group; the store map lane (rank j = 16 sl + jj, columns
    n .. n + 3, n = col0 + 16 nt + 4 q) into D[r, K] (RK) or D[K, r] (KR).  Ranks at or past r are never stored: the
    accumulators of those lanes are returned in `dead` (they must be zero)."""
    M, K = X.shape
    r = T.shape[1]
    ns = (r + 15) // 16
    D = np.full((r, K) if layout == "RK" else (K, r), np.nan)
    dead = []
    for col0 in range(0, K, 32):
        acc = [[np.zeros((64, 4)) for _ in range(ns)] for _ in range(2)]
        for m0 in range(0, M, 32):
            for sl in range(ns):
                step = colreduce16_step(X[m0:m0 + 32, col0:col0 + 32], T[m0:m0 + 32], sl, split)
                for nt in range(2):
                    acc[nt][sl] += step[nt]
        for sl in range(ns):
            for l in range(64):
                jj, q = l & 15, l >> 4
                j = 16 * sl + jj
                for nt in range(2):
                    if j >= r:
                        dead.append(acc[nt][sl][l])
                        continue
                    for reg in range(4):
                        nn = col0 + 16 * nt + 4 * q + reg
                        if layout == "RK":
                            D[j, nn] = acc[nt][sl][l][reg]
                        else:
                            D[nn, j] = acc[nt][sl][l][reg]
    return D, np.array(dead)


def check_colreduce16():
    rng = np.random.default_rng(1)
    for r, M in ((9, 32), (17, 45), (64, 70)):   # whole steps; a ragged last step; three steps, four slices
        X = bf16_round(rng.standard_normal((M, 64)).astype(np.float32))
        T = rng.standard_normal((M, r)).astype(np.float32).astype(np.float64)
        for layout in ("RK", "KR"):
            D, dead = colreduce16(X, T, layout)
            want = T.T @ X
            assert np.allclose(D, want if layout == "RK" else want.T)
            assert not np.isnan(D).any() and not dead.any() and (len(dead) > 0) == (r % 16 != 0)
        # hi + lo: T to ~16 mantissa bits, against 8 for hi alone
        Ds, _ = colreduce16(X, T, "RK", split=True)
        bound = np.abs(T).T @ np.abs(X)
        assert np.all(np.abs(Ds - T.T @ X) <= 2.0 ** -15 * bound)
        hi, lo = split_hi_lo(T)
        assert np.allclose(Ds, (hi + lo).T @ X, rtol=0, atol=1e-12 * bound.max())
        assert np.abs(hi.T @ X - T.T @ X).max() > 2.0 ** -15 * bound.max()
    return True


def rank_update16_rows(T, U, scale=1.0, row_scale=None, nsel=1, rps=1, m0=0):
    """rank_update16_mfma_kernel on the rows m0 .. m0 + len(T) - 1 of one 32-column group, as a workgroup walks them: 16-row
    slabs (the last one ragged), NS = ceil(r / 16) slices chained into the same two accumulators, T and U as hi + lo fragments
    (k = 32 holds (hi | lo) of U's 16 ranks against T's hi twice, then T's lo twice).  T: [rows, r] f32 values, U: [32, r].
    row_scale [nsel, r] (the row-table form, lora_amd_rank_update_rowscale): the lane of row m looks its table row
    (m // rps) % nsel up ONCE per slab, and every slice multiplies its eight T values by that row's entries in f32 before the
    split.  Returns scale * (T o row_scale[q]) U^T [rows, 32] (the accumulators in float64; `scale` is the epilogue's
    multiplier, applied as f32)."""
    rows, r = T.shape
    ns = (r + 15) // 16
    T32 = np.asarray(T, np.float32)
    RS32 = None if row_scale is None else np.asarray(row_scale, np.float32)
    ua = [[None, None] for _ in range(ns)]
    for sl in range(ns):
        for tile in range(2):
            v = np.zeros((64, 8))
            for l in range(64):
                mm, q = l & 15, l >> 4
                n = 8 * (mm >> 2) + 4 * tile + (mm & 3)
                for e in range(8):
                    j = 16 * sl + 8 * (q & 1) + e
                    v[l][e] = U[n, j] if j < r else 0.0
            hi, lo = split_hi_lo(v)
            ua[sl][tile] = np.where((KQ < 2)[:, None], hi, lo)
    out = np.zeros((rows, 32))
    for s0 in range(0, rows, 16):
        d = [np.zeros((64, 4)), np.zeros((64, 4))]
        sample = [((m0 + s0 + mm) // rps) % nsel for mm in range(16)]   # per lane and slab, ahead of the slices
        for sl in range(ns):
            v = np.zeros((64, 8), np.float32)
            for l in range(64):
                mm, q = l & 15, l >> 4
                if s0 + mm >= rows:
                    continue
                for e in range(8):
                    j = 16 * sl + 8 * (q & 1) + e
                    if j < r:
                        v[l][e] = T32[s0 + mm, j]
                        if RS32 is not None:
                            v[l][e] = np.float32(v[l][e] * RS32[sample[mm], j])
            th, tl = split_hi_lo(v)
            for tile in range(2):
                d[tile] = mfma(ua[sl][tile], th, d[tile])
                d[tile] = mfma(ua[sl][tile], tl, d[tile])
        for l in range(64):
            mm, q = l & 15, l >> 4
            if s0 + mm < rows:
                out[s0 + mm, 8 * q:8 * q + 4] = d[0][l]
                out[s0 + mm, 8 * q + 4:8 * q + 8] = d[1][l]
    return np.float64(np.float32(scale)) * out


def check_rank_update16_rows():
    """the wide and the row-table staging against float64 (hi + lo on both operands: the 2^-15 of check_colreduce16), and
    the two bit rules of the table: all ones -> the plain form's bits; a constant power of two c per sample -> the plain
    form at scale c on that sample's rows"""
    rng = np.random.default_rng(2)
    for r, rows, nsel, rps, m0 in ((9, 16, 2, 5, 0), (17, 23, 3, 7, 64), (64, 40, 2, 13, 128)):
        T = rng.standard_normal((rows, r)).astype(np.float32)
        U = rng.standard_normal((32, r)).astype(np.float32).astype(np.float64)
        RS = (rng.random((nsel, r)) * 2 - 0.5).astype(np.float32)
        q = ((m0 + np.arange(rows)) // rps) % nsel
        TS = T.astype(np.float64) * RS.astype(np.float64)[q]
        got = rank_update16_rows(T, U, 0.75, RS, nsel, rps, m0)
        assert np.all(np.abs(got - 0.75 * TS @ U.T) <= 2.0 ** -15 * 0.75 * (np.abs(TS) @ np.abs(U).T))
        plain = rank_update16_rows(T, U, 0.75)
        assert np.all(np.abs(plain - 0.75 * T.astype(np.float64) @ U.T) <= 2.0 ** -15 * 0.75 * (np.abs(T) @ np.abs(U).T))
        assert np.array_equal(rank_update16_rows(T, U, 0.75, np.ones((nsel, r)), nsel, rps, m0), plain)
        c = np.array([2.0, 0.5, 1.0])[:nsel]
        got = rank_update16_rows(T, U, 0.75, np.repeat(c[:, None], r, 1), nsel, rps, m0)
        for k in range(nsel):
            assert np.array_equal(got[q == k], rank_update16_rows(T, U, 0.75 * c[k])[q == k])
    return True


def check():
    rng = np.random.default_rng(0)
    for r in (16, 12, 9):
        T, U = rng.standard_normal((16, r)), rng.standard_normal((32, r))
        assert np.allclose(rank_update16(T, U), T @ U.T)
        G, T32, U32 = rng.standard_normal((32, 32)), rng.standard_normal((32, r)), rng.standard_normal((32, r))
        gt, dup = bwd_g16_unit(G, T32, U32)
        assert np.allclose(gt[:, :r], G @ U32) and not gt[:, r:].any()
        assert np.allclose(dup[:, :r], G.T @ T32) and not dup[:, r:].any()
        X, F = rng.standard_normal((16, 32)), rng.standard_normal((r, 32))
        t = rowdot16_step(X, F)
        assert np.allclose(t[:, :r], X @ F.T) and not t[:, r:].any()
    return True


if __name__ == "__main__":
    print("ok" if check() and check_colreduce16() and check_rank_update16_rows() else "mismatch")
