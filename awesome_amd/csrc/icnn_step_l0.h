// icnn_step_l0.h - one slice (r, k) of the layer-0 gradient of icnn_step_kernel's main units, a block of its code (no header of its own
// right: icnn_step.h includes it where the slices run, between the k-steps of the dW product).  `r` and `k` are compile-time constants
// at the place of inclusion.  Slice (r, 0) first transposes index r of the masked dz0 between lane groups and tiles - D[q][j] = dz0 of
// unit (4q + g, l15) at point 4j + r, eight permlane swaps per tile quad - then every slice adds point 4k + r to the NEXT chains of
// each quad: dL0[q][0] += D, dL0[q][1 + c] += D x_c, with the point's coordinates in xpq[k][] (requested earlier from stage B).
// The slices run r-major, then k: the order in which the matrix pipe would add the 16 points of the wave.
                    if (k == 0) {
#pragma unroll
                        for (int q = 0; q < NQ; ++q) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) D[q][j] = 4 * q + j < TM ? dz0[4 * q + j < TM ? 4 * q + j : 0][r] : 0.f;
                            swap32(D[q][0], D[q][2]);
                            swap32(D[q][1], D[q][3]);
                            swap16(D[q][0], D[q][1]);
                            swap16(D[q][2], D[q][3]);
                        }
                    }
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        dL0[q][0] += D[q][k];
#pragma unroll
                        for (int c = 0; c < C; ++c) dL0[q][1 + c] = fmaf(D[q][k], xpq[k][c], dL0[q][1 + c]);
                    }
