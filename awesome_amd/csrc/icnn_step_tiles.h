// icnn_step_tiles.h - the dW tile stores of icnn_step_kernel, a block of its code behind the chunk loop (no header of its own right:
// icnn_step.h includes it at every place where tiles leave).  `slab` is this workgroup's gradient slab; the tiles (row tile j, column
// tile b) with tile_from <= j KG + b < tile_to are stored, and nothing is scheduled across the block.
        __builtin_amdgcn_sched_barrier(0);
        if (row_ok) {
#pragma unroll
            for (int j = 0; j < RPW; ++j) {
#pragma unroll
                for (int b = 0; b < KG; ++b) {
                    bool used = true;   // the last column tile holds the leftover units and the ext inputs only: skip its padding
                    if (b == KG - 1) {
                        used = l15 < HR;
#pragma unroll
                        for (int e = 0; e < NEXT; ++e) used = used || (HM + l15 == G::ext_pos(e));
                    }
                    if (used && j * KG + b >= tile_from && j * KG + b < tile_to) {
                        f32x4* dst = (f32x4*)(slab + ((((wave * RPW + j) * KG + b) * 64 + lane) << 2));
                        __builtin_nontemporal_store(dW[j][b], dst);   // written once, read once by another kernel
                    }
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#if INR_STAMPS
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_store)::"memory");   // a tile store has been issued (the last one's stays)
        __builtin_amdgcn_sched_barrier(0);
#endif
