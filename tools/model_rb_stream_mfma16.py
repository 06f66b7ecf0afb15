"""CPU model of the lane maps of k_rb_stream on v_mfma_f32_16x16x32 (csrc/mfma_conv.hpp kconv16, csrc/rb_stream_kernels.hpp SH = 16), a sibling of
tools/model_rb_stream.py, whose row-level schedule it re-runs with every register tile held lane by lane.  Three things, each a function a test calls
(tests/test_cpu_rb_stream_mfma16.py):

  kloop_products   walks kconv16's A gathers (raw buffer offsets into the packed weights [co_tile][k_step][lane][8]) and B reads (LDS byte addresses)
                   MFMA by MFMA and counts, per output (channel, row), which (input channel, tap) products the instruction forms
  bank_slots       the 16-byte LDS slots (modulo 256 B) that each ds_read_b128 lane group of a B read touches
  run_strip16      model_rb_stream.run_strip with xin / res / carry / h / acc as [wave][half][tile][lane][4] arrays: T pick-up and deposit, publish,
                   dual write, H tail, the residual shift by two tiles and the two-tile carry, the first step's fill tiles (2 (m + 1) on) poisoned

The MFMA itself (what the hardware defines): A lane (q, n) = (lane // 16, lane % 16) holds A[n][8 q .. 8 q + 8], B lane (q, n) holds B[8 q .. 8 q + 8][n],
D lane (q, n) holds D[4 q .. 4 q + 4][n], D = A B summed over the 32 k.
Run: python tools/model_rb_stream_mfma16.py"""
import numpy as np

import model_rb_stream as base

C = 128
STRIDE = 2 * C + 16           # bytes per LDS operand row
NJ = 6
R = 32 * NJ
NT = 2 * NJ                   # column tiles of 16 rows
# the ds_read_b128 lane groups of gfx950 (one LDS cycle each)
LANE_GROUPS = [[g + 32 * u for g in grp] for u in (0, 1) for grp in ((0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27),
                                                                   (4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31))]


def mfma16_row(n):
    return 2 * n if n < 4 else 2 * n - 7 if n < 12 else 2 * n - 16


def mfma16_chunk(q):
    return ((q & 1) << 1) | (q >> 1)


def mfma16_loff(lane):
    q, n = lane >> 4, lane & 15
    return ((q & 1) * 64 + (q >> 1) * 32 + n) * 16


def b_address(lane, row0, natural=False):
    """LDS byte address of this lane's B fragment at tap 0, 32-k step 0, tile 0 (kconv16's lds_row); natural = the assignment that conflicts"""
    q, n = lane >> 4, lane & 15
    return (row0 + (n if natural else mfma16_row(n))) * STRIDE + (q if natural else mfma16_chunk(q)) * 16


def bank_slots(natural=False):
    """-> for every B read of a k = 11, dilation 5 conv (every tap, 32-k step and tile) and every lane group: the slots modulo 256 B"""
    out = []
    for tap in range(11):
        for s in range(4):
            for jt in range(NT):
                for grp in LANE_GROUPS:
                    out.append([((b_address(l, 3, natural) + tap * 5 * STRIDE + s * 64 + jt * 16 * STRIDE) // 16) % 16 for l in grp])
    return out


def kloop_products(k, dil, jt0=0):
    """-> cnt[co 32][row R][ci C][tap k]: how often kconv16 forms the product W[co][ci][tap] * X[row + tap * dil][ci] into output (co, row) of one wave.
    The packed weight buffer holds element (co, tap * C + ci) of the wave's tile at [k_step = (tap * C + ci) // 16][lane = (co % 32) + 32 * ((ci % 16) // 8)][ci % 8]
    (csrc/mfma_conv.hpp, "A (weights)"); X row r, channel ci is at LDS byte r * STRIDE + 2 * ci."""
    cnt = np.zeros((32, R, C, k), np.int32)
    lanes = np.arange(64)
    q, n = lanes >> 4, lanes & 15
    loff = np.array([mfma16_loff(l) for l in lanes])
    lds_row = np.array([b_address(l, 0) for l in lanes])
    e = np.arange(8)
    for g in range(k):                       # C = 128: a group of 8 k-steps is one tap
        soff = g * 8192
        for s in range(4):
            for jt in range(jt0, NT):
                baddr = lds_row + g * dil * STRIDE + s * 64 + jt * 16 * STRIDE          # [lane]
                brow, bci = baddr // STRIDE, (baddr % STRIDE) // 2                      # first of the lane's 8 channels
                assert (baddr % STRIDE + 16 <= 2 * C).all()                             # never the row pad
                for h in range(2):
                    aoff = (soff + loff + s * 2048 + h * 256) // 16                     # [lane] in 16-byte fragments = k_step * 64 + packed lane
                    kstep, plane = aoff // 64, aoff % 64
                    aco = plane & 31                                                    # A row n of the instruction
                    akk = 16 * kstep[:, None] + 8 * (plane >> 5)[:, None] + e[None]     # [lane][8] k index = tap * C + ci
                    # the instruction: D[m][col] += sum over K-blocks qq, e of A(lane (qq, m)) * B(lane (qq, col))
                    for qq in range(4):
                        la = 16 * qq + np.arange(16)                                    # the 16 lanes of K-block qq (index = m for A, = col for B)
                        co = aco[la]                                                    # [m]
                        assert (co == 16 * h + np.arange(16)).all()
                        atap, aci = akk[la] // C, akk[la] % C                           # [m][8]
                        assert (atap == g).all()
                        rows = brow[la] - g * dil                                       # [col] output row
                        assert (rows == 16 * jt + np.array([mfma16_row(c) for c in range(16)])).all()   # = the D lane's row (ROW_OF, below)
                        assert (aci[0] == bci[la][0] + e).all() and (aci == aci[0]).all() and (bci[la] == bci[la][0]).all()
                        np.add.at(cnt, (co[:, None, None], rows[None, :, None], aci[0][None, None, :], g), 1)
    return cnt


# ---- the step schedule with lane-held tiles ------------------------------------------------------------------------------------------
LROW = np.array([mfma16_row(l & 15) for l in range(64)])
ROW_OF = (16 * np.arange(NT)[:, None] + LROW[None, :])                                   # [tile][lane]
# [wave][half][lane][e] -> channel: 32 wave + 16 half + 4 (lane // 16) + e
CH_OF = (32 * np.arange(4)[:, None, None, None] + 16 * np.arange(2)[None, :, None, None] + 4 * (np.arange(64) >> 4)[None, None, :, None]
         + np.arange(4)[None, None, None, :])


def to_lanes(X):
    """rows x C (the transposition tile T, or a conv's D) -> [wave][half][tile][lane][e]"""
    return X[ROW_OF[None, None, :, :, None], CH_OF[:, :, None, :, :]].astype(np.float32)


def scatter(dst, row0, tiles, lanes_val, mask_rows=None, first_row=0, nrows=None):
    """publish / deposit: tile jt of `tiles`, lane l, quad e -> dst[row0 + 16 jt + lrow - first_row][channel], rows outside [0, nrows) dropped (the dump row)"""
    for jt in tiles:
        r = ROW_OF[jt] - first_row                                                       # [lane]
        ok = (r >= 0) & ((r < nrows) if nrows is not None else True)
        v = lanes_val[:, :, jt]                                                          # [wave][half][lane][e]
        if mask_rows is not None:
            v = np.where(mask_rows[jt][None, None, :, None], v, 0)
        for l in np.nonzero(ok)[0]:
            dst[row0 + r[l], CH_OF[:, :, l, :]] = v[:, :, l, :]


def run_strip16(x, W1, B1, W2, B2, k, dils, S0, S1, out, fill=True):
    L = x.shape[0]
    nd = len(dils)
    HEAD, HROW, SLACK, lrelu = base.HEAD, base.HROW, base.SLACK, base.lrelu
    p2 = (k - 1) // 2
    p1 = [d * (k - 1) // 2 for d in dils]
    Hx = [32 + p - p2 for p in p1]
    r0 = S0 - (sum(p1) + nd * p2)
    nsteps = -(-(S1 - r0 + 32 * nd) // R)
    M = np.zeros((HEAD + R + SLACK, C), np.float32)
    sideX = [np.zeros((Hx[m], C), np.float32) for m in range(nd)]
    sideH = [np.zeros((2 * p2, C), np.float32) for m in range(nd)]
    carry = [np.zeros((4, 2, 2, 64, 4), np.float32) for m in range(nd)]                  # two tiles
    for i in range(nsteps):
        rows = r0 + i * R + np.arange(R)
        T = np.where(((rows >= 0) & (rows < L))[:, None], x[np.clip(rows, 0, L - 1)], 0).astype(np.float32)   # the load descriptor's range check
        xin = to_lanes(T)                                                                # D-layout pick-up
        for m in range(nd):
            wm = r0 - 32 * m + i * R
            M[HEAD - Hx[m]:HEAD] = sideX[m]                                              # X head restored (row-wise, wave-private)
            M[HROW - 2 * p2:HROW] = sideH[m]
            t = wm + ROW_OF
            mask = (t >= 0) & (t < L)                                                    # [tile][lane]
            act = lrelu(xin)
            scatter(M, HEAD, range(NT), act, mask)                                       # publish
            scatter(sideX[m], 0, range(NT - 4, NT), act, mask, first_row=R - Hx[m], nrows=Hx[m])   # dual write: the tiles of the last 64 rows
            res = np.concatenate([carry[m], xin[:, :, :NT - 2]], axis=2)                 # res[jt] = xin[jt - 2]
            carry[m] = xin[:, :, NT - 2:].copy()
            jt0 = 2 * (m + 1) if (fill and i == 0 and m + 1 <= NJ - 2) else 0            # LAG * rs_fill_inst(m, NJ)
            b0 = HEAD - Hx[m]
            h = np.tile(B1[m][None, :], (R, 1)).astype(np.float32)
            for j in range(k):
                h += M[b0 + j * dils[m]: b0 + j * dils[m] + R] @ W1[m][:, :, j].T
            hl = to_lanes(h)
            hl[:, :, :jt0] = np.nan                                                      # not computed: bias only in the kernel, read by nothing
            t = wm - 32 + p2 + ROW_OF
            mask = (t >= 0) & (t < L)
            act = lrelu(hl)
            scatter(M, HROW, range(NT), act, mask)
            scatter(sideH[m], 0, range(NT - 2, NT), act, mask, first_row=R - 2 * p2, nrows=2 * p2)   # H tail: the tiles of the last 32 rows
            b0 = HROW - 2 * p2
            acc = np.zeros((R, C), np.float32)
            for j in range(k):
                acc += M[b0 + j: b0 + j + R] @ W2[m][:, :, j].T
            xin = (res + B2[m][CH_OF][:, :, None]) + to_lanes(acc)
            xin[:, :, :jt0] = np.nan
        T = np.full((R, C), np.nan, np.float32)
        scatter(T, 0, range(NT), xin)                                                    # deposit (a row never written, or a poisoned one, stays NaN)
        rows = r0 - 32 * nd + i * R + np.arange(R)
        ok = (rows >= S0) & (rows < S1)
        out[rows[ok]] = T[ok]


def strip_case(k, dils, L, strips, seed=0):
    """-> (lane-level result, direct ResBlock1) of one resblock over `strips` strips"""
    rng = np.random.default_rng(seed)
    nd = len(dils)
    W1 = [rng.standard_normal((C, C, k), dtype=np.float32) / np.float32(np.sqrt(C * k)) for _ in range(nd)]
    W2 = [rng.standard_normal((C, C, k), dtype=np.float32) / np.float32(np.sqrt(C * k)) for _ in range(nd)]
    B1 = [(rng.standard_normal(C, dtype=np.float32) * np.float32(0.1)).astype(np.float32) for _ in range(nd)]
    B2 = [(rng.standard_normal(C, dtype=np.float32) * np.float32(0.1)).astype(np.float32) for _ in range(nd)]
    x = rng.standard_normal((L, C), dtype=np.float32)
    out = np.full((L, C), np.nan, np.float32)
    sl = -(-L // strips)
    for s in range(strips):
        run_strip16(x, W1, B1, W2, B2, k, dils, s * sl, min(L, (s + 1) * sl), out)
    return out, base.reference(x, W1, B1, W2, B2, k, dils)


def main():
    for grp in bank_slots():
        assert len(set(grp)) == 16, grp
    assert any(len(set(grp)) < 16 for grp in bank_slots(natural=True))
    for k, dil in ((3, 1), (7, 3), (11, 5)):
        assert (kloop_products(k, dil) == 1).all()
    for k in (3, 7, 11):
        for L, strips in ((700, 1), (700, 2), (90, 1)):
            got, ref = strip_case(k, [1, 3, 5], L, strips)
            assert np.isfinite(got).all() and np.abs(got - ref).max() < 2e-4, (k, L, strips, np.abs(got - ref).max())
    print("kconv16: every product once, 16 slots per lane group; lane-held step schedule == direct ResBlock1 (fill tiles poisoned)")


if __name__ == "__main__":
    main()
