// icnn_step_bwd.h - the backward block of icnn_step_kernel for one wave's 16 points of a chunk, a block of its code (no header of its own
// right: icnn_step.h includes it once, inside the wave-uniform `if (live_w)` behind the data term).  dz1 with its staging and the dw_o
// sums, the backward product dZ0 = dZ1 . W1 with the layer-0 mask, the leftover rows of the layer-0 gradient and (DX) dL/dcoords.
// A wave whose 16 dy are all +-0 does not run it: every sum in here would add +-0 ("chunks without a gradient").
// It is a file and not a lambda for the reason icnn_step_tiles.h is: as a lambda over dz0 it moves hipcc's allocation of the kernel.
                // dz1 of tile t (in place over acc), dw_o accumulation, staging of dz1 (A)
                auto dz1_tile = [&](int t) {
                    const f32x4 wot = wo[t];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float z1 = acc[t][r];
                        dwo[t][r] = fmaf(dy, z1, dwo[t][r]);
                        acc[t][r] = z1 > 0.f ? dy * wot[r] : 0.f;
                    }
                    *(f32x4*)(sa + 16 * t) = acc[t];
                };

                STAMP(3);
                // ---- backward through layer 1 (MFMA, pipelined): dZ0 = dZ1 . W1 ----------------------------------------
                // Operands swapped w.r.t. the forward product (same registers): the D tile comes out transposed - rows =
                // this wave's points 4g+r, columns = hidden unit 16t + l15 - so every lane holds dz0 of ONE hidden unit per tile for
                // four of the wave's own points: the layer-0 gradient dW_in = dZ0^T . (1, x) is per-lane FMAs, no staging, no barrier.
                f32x4 dzx = f32x4{0.f, 0.f, 0.f, 0.f};  // DX: same product for the columns of k-group TM (skip-path inputs)
                float bqx[2] = {0.f, 0.f};
                float dz0l[HRA];
#pragma unroll
                for (int u = 0; u < HRA; ++u) dz0l[u] = 0.f;
                // k-steps over the hidden outputs.  The HR <= 4 leftover outputs share ONE k-step: dzl[] is the same in all four lane
                // groups, so lane group u < HR carries leftover unit u (operand dzl[u], weight row HM + u), the others feed zeros.
                constexpr int KS = 4 * TM + (HR > 0 ? 1 : 0);
                float dzlg = 0.f;   // this lane group's leftover dz1
#pragma unroll
                for (int u = 0; u < HR; ++u) dzlg = g == u ? dzl[u] : dzlg;
                float bq[2][TM];      // B operands (weights): row o of this k-step, columns 16t + l15
                f32x4 wcq[2][HRA];    // leftover input columns W1[o][HM+u] at this lane's positions of a tile
                auto b_row = [&](int ks) -> const float* {  // LDS row of the weight operand for k-step ks
                    const int tk = ks >> 2, r = ks & 3;
                    if (tk < TM) return wb + (16 * tk + 4 * g + r) * S;
                    return wb + (g < HR ? (HM + g) * S : 0);  // leftover output u lives in lane group u (others: A = 0)
                };
                // relu nets: the layer-0 mask is the sign of z0, unit 16t + l15 at point 4g + r, read back from this wave's own stage-B rows
                // (written by this wave in the forward product; the b32 pattern of the dW product's bf reads, conflict-free).  One read
                // behind every second product of the last eight k-steps: requested late, and no wait in front of an MFMA.
                f32x4 zm[TM];
                const float* const zrow = stB + (wave * 16 + 4 * g) * G::SB + l15;
                constexpr int MK0 = KS > 8 ? KS - 8 : 0;   // first k-step that carries mask reads
                auto mask_read = [&](int i) {
                    if (MASK_STAGED && i < 4 * TM) zm[i % TM][i / TM] = zrow[(i / TM) * G::SB + 16 * (i % TM)];
                };
                dz1_tile(0);
                {
                    const float* br = b_row(0);
#pragma unroll
                    for (int t = 0; t < TM; ++t) bq[0][t] = br[16 * t];
                    if (DX) bqx[0] = br[16 * TM];
#pragma unroll
                    for (int u = 0; u < HR; ++u) wcq[0][u] = *(const f32x4*)(WcT + u * PT + 4 * g);
                }
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const int tk = ks >> 2, r = ks & 3;
                    if (ks + 1 < KS) {
                        const float* br = b_row(ks + 1);
                        if (DX) bqx[(ks + 1) & 1] = br[16 * TM];
                    }
                    if (r == 0 && (tk + 1) * 4 < KS) {
#pragma unroll
                        for (int u = 0; u < HR; ++u) wcq[(tk + 1) & 1][u] = *(const f32x4*)(WcT + u * PT + 16 * (tk + 1) + 4 * g);
                    }
                    OPERAND_FENCE();
                    const float bop = tk < TM ? acc[tk < TM ? tk : 0][r] : dzlg;
#pragma unroll
                    for (int t = 0; t < TM; ++t) {  // D = dZ0 with POINTS on the rows; next k-step's operand reads one per product
                        dz0[t] = MFMA16(bop, bq[ks & 1][t], ks == 0 ? (f32x4{0.f, 0.f, 0.f, 0.f}) : dz0[t]);
                        if (ks + 1 < KS) bq[(ks + 1) & 1][t] = b_row(ks + 1)[16 * t];
                        if (ks >= MK0 && (((ks - MK0) * TM + t) & 1)) mask_read(((ks - MK0) * TM + t) >> 1);
                        OPERAND_FENCE();
                    }
                    if (DX) dzx = MFMA16(bop, bqx[ks & 1], dzx);
                    MFMA_STEP_FENCE();
                    if (r == 1 && tk + 1 < TM) dz1_tile(tk + 1);  // next tile's dz1 + staging, in the shadow of the MFMAs
                    // leftover hidden inputs: dz0l[u] += W1[:, HM+u] . dz1 - this k-step's share (HR FMAs per MFMA block, not 4 HR
                    // in one gap every fourth block)
#pragma unroll
                    for (int u = 0; u < HR; ++u) {
                        if (tk < TM) dz0l[u] = fmaf(wcq[tk & 1][u][r], acc[tk < TM ? tk : 0][r], dz0l[u]);
                        else if (g == 0) {   // the leftover outputs' share stays ONE chain in lane group 0 (output HM + 0, then HM + 1, ..)
#pragma unroll
                            for (int v = 0; v < HR; ++v) dz0l[u] = fmaf(wcq[tk & 1][u][v], dzl[v], dz0l[u]);
                        }
                    }
                    MFMA_STEP_FENCE();
                }
                STAMP(4);
                // Layer-0 derivative (relu nets: the mask zm read from stage B; encode nets: z0p, computed before the output layer); then the
                // layer-0 gradient dW_in += dZ0^T . (1, x) over this wave's 16 points.  On the VALU: the product has NEXT useful columns, a
                // matrix-pipe tile pads them to 16 (4 TM MFMAs for 6 MFMAs' worth of arithmetic).  dz0[t][r] holds point
                // 4g + r of unit (t, l15); a 4 x 4 transpose between lane groups and tiles (four permlane swaps per four registers) hands
                // lane group g the tiles 4q + g for the points of ALL lane groups, and every parameter is then one FMA chain in the matrix
                // pipe's own order: the same bits as the MFMA form.  Nothing in front of the chunk-end barrier needs these sums, and the
                // block is latency, not issue (six dependent chains): only the mask is applied here, the transpose and the chains run as 16
                // slices behind the k-steps of the dW product below (icnn_step_l0.h), r-major, then k - every chain adds in the same order.
#pragma unroll
                for (int i = (KS - MK0) * TM / 2; i < 4 * TM; ++i) mask_read(i);   // (shapes with fewer than eight k-steps)
#pragma unroll
                for (int t = 0; t < TM; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if constexpr (MASK_STAGED) dz0[t][r] = zm[t][r] > 0.f ? dz0[t][r] : 0.f;
                        else dz0[t][r] *= dact0_f<ACT0>(z0p[t][r], a.act_omega);
                    }
                // leftover rows of the layer-0 gradient (lane group 0, VALU)
                float hx[C];  // DX: the contributions that live per point on lane l15: s_o dy + W_in[HM+u] dz0l[u]
#pragma unroll
                for (int c = 0; c < C; ++c) hx[c] = s_o[c] * dy;
#pragma unroll
                for (int u = 0; u < HR; ++u) {
                    const float d = sum_over_groups(dz0l[u]);
                    // position HM + u lives in lane group 0, k-step u (DX needs it in every lane group)
                    const float z0u = DX ? __shfl(z0[TM][u], l15) : z0[TM][u];
                    float dm;
                    if constexpr (ACT0 == INR_ACT_RELU) dm = z0u > 0.f ? d : 0.f;
                    else dm = d * dact0_f<ACT0>(z0lpre[u], a.act_omega);   // (used in lane group 0 only, where z0lpre[u] is unit HM + u)
                    if (DX) {
#pragma unroll
                        for (int c = 0; c < C; ++c) hx[c] = fmaf(WinT[c * 16 + u], dm, hx[c]);
                    }
                    if (g == 0) {
                        dL0l[u][0] += dm;
#pragma unroll
                        for (int c = 0; c < C; ++c) dL0l[u][1 + c] = fmaf(dm, x[c], dL0l[u][1 + c]);
                    }
                }
                if (DX) {
                    // dL/dx_c of point 4g + r: sum over hidden units (lanes l15, tiles t) of W_in[.,c] dz0, plus the skip
                    // path (column ext_pos(1+c) of the transposed product dzx), plus the per-point terms of that point.
                    float part[4][C];
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int c = 0; c < C; ++c) part[r][c] = (l15 == G::ext_pos(1 + c) - HM) ? dzx[r] : 0.f;
#pragma unroll
                    for (int t = 0; t < TM; ++t)
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            const float w = WinE[c * PT + bcol(t, l15)];
#pragma unroll
                            for (int r = 0; r < 4; ++r) part[r][c] = fmaf(w, dz0[t][r], part[r][c]);
                        }
                    // lane (g, l15 = r) keeps the value of point 4g + r: C coalesced stores per wave instead of 4C masked ones
                    float dxv[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) dxv[c] = 0.f;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            const float v = sum_over_points(part[r][c]);   // in every lane of the lane group
                            dxv[c] = l15 == r ? v : dxv[c];
                        }
                    const int pp = chunk * SP + wave * 16 + 4 * g + l15;
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const float v = dxv[c] + __shfl(hx[c], 4 * g + l15);   // hx lives on lane (0, point)
                        if (l15 < 4 && pp < (int)N) a.dcoords[((size_t)img * C + c) * N + pp] = v;
                    }
                }
