/* substep_g's limit-row solves (speculative / partial solve, the check, the all-rows redo): the
 * text of one instance, included by pgx_kernels.hip where `mgi_c` (IC<1>: the merged wave's
 * instance, IC<0>: the two-register one) and substep_g's locals are in scope.  Kernels without
 * merged sweeps include it in place, as plain statements of substep_g: wrapped in a lambda the
 * object kernels' unit compiled to other code (Push 4096 +1.4 %). */
            constexpr bool MGI = decltype(mgi_c)::value != 0;
            /* (lanes MG0.. only: independent of the slot mirrors below, which write lane SL0) */
            if constexpr (MGI) merge_rows();
            const float gm0 = gv;   /* MGI: the merged start (gv0 and gw0 are then dead through the sweeps) */
            if (PART && !NO_PART && !spec_all && nk <= KMAX && nxr == 0) {   /* (NO_PART: all rows instead, fewer registers) */
                PGX_PROF_COUNT(7, 1);
                /* slots in the pairs' table order; slot lane SL0 + S mirrors dof d_S */
                int ds[2] = {0, 0};
                int k = 0;
                sfor<0, (PGX_N_ROWS - NJ) / 2>([&](auto pc) __attribute__((always_inline)) {
                    constexpr int d = kPgxRowCode[NJ + 2 * decltype(pc)::value] & 15;
                    if ((dmask >> d) & 1u) { if (k == 0) ds[0] = d; else ds[1] = d; k++; }
                });
                ds[0] = __builtin_amdgcn_readfirstlane(ds[0]);
                ds[1] = __builtin_amdgcn_readfirstlane(ds[1]);
                const int src = (int)(threadIdx.x & ~(unsigned)(GW - 1));
                auto mirror = [&](float& x) __attribute__((always_inline)) {
                    x = lane_sel<SL0>(__shfl(x, src + ds[0]), x);
                    if (KMAX > 1 && nk > 1) x = lane_sel<SL0 + 1>(__shfl(x, src + ds[1]), x);
                };
#pragma unroll
                for (int d = 0; d < NJ; d++) {
                    if constexpr (PKM) {   /* (mcs / cR live on only as the pairs' halves) */
                        float t = mw[d].x;
                        mirror(t);
                        mw[d].x = t;
                    } else {
                        mirror(mcs[d]);
                    }
                }
                mirror(gv);
                if (g1_any) {
#pragma unroll
                    for (int p = 0; p < NP; p++)
#pragma unroll
                        for (int dir = 0; dir < 3; dir++) {
                            if constexpr (PKC) {
                                float t = crw[3 * p + dir].x;
                                mirror(t);
                                crw[3 * p + dir].x = t;
                            } else {
                                mirror(cR[p][dir]);
                            }
                        }
                }
                /* the slots' row data: dof d_S's entries, selected with uniform masks */
#pragma unroll
                for (int S = 0; S < KMAX; S++) {
                    if constexpr (PKM) smw[S] = mw[0];
                    else { smcs[S] = mcs[0]; if constexpr (!MGI) swms[S] = PKD ? mw2[0].x : wms[0]; }
                    if constexpr (!MGI) swms2[S] = PKD ? mw2[0].y : wms2[0];
                    slhi[S] = lhi[0];
                    srh[S][0] = rl[0]; srh[S][1] = ru[0];
                    slam[S][0] = 0.0f; slam[S][1] = 0.0f;
                    sfor<1, NJ>([&](auto dc) __attribute__((always_inline)) {
                        constexpr int d = decltype(dc)::value;
                        const bool hit = ds[S] == d;   /* wave-uniform */
                        auto sel = [&](float a, float o) __attribute__((always_inline)) { return hit ? a : o; };
                        if constexpr (PKM) smw[S] = hit ? mw[d] : smw[S];
                        else { smcs[S] = sel(mcs[d], smcs[S]); if constexpr (!MGI) swms[S] = sel(PKD ? mw2[d].x : wms[d], swms[S]); }
                        if constexpr (!MGI) swms2[S] = sel(PKD ? mw2[d].y : wms2[d], swms2[S]);
                        slhi[S] = sel(lhi[d], slhi[S]);
                        srh[S][0] = sel(rl[d], srh[S][0]); srh[S][1] = sel(ru[d], srh[S][1]);
                    });
                }
                /* the checks skip the running dofs and the slot lanes */
                if ((dmask >> c) & 1u) { rl_c = -3.0e38f; ru_c = -3.0e38f; }
                if (c == SL0) rcol = ds[0];
                if (KMAX > 1 && nk > 1 && c == SL0 + 1) rcol = ds[1];
                PGX_PROF_COUNT(16, nk == 2 ? 1 : 0);
                PGX_PROF_COUNT(18, any_contact ? 1 : 0);
                if (KMAX == 1 || nk == 1) solve_w(IC<3>{}, IC<1>{}, mgi_c);
                else solve_w(IC<3>{}, IC<KMAX>{}, mgi_c);
            } else if (spec_all) {
                solve_w(IC<1>{}, IC<0>{}, mgi_c);
            } else {
                lmargin = -1.0f;   /* more than KMAX dofs: all rows */
            }
            const bool viol = lmargin < 0.0f;
            if (__any(row_any(viol)) || e.pgs_mode == 3) {
                PGX_PROF_COUNT(12, 1);
                if constexpr (MGI) {
                    split_rows();
                    gv = gm0;
                    gw = hi_sel(0.0f, ror8(gm0));
                } else {
                    gv = gv0;
                    gw = gw0;
                    gw2 = gw20;
                }
#pragma unroll
                for (int p = 0; p < NP; p++) {
                    clam[p][0] = CONT ? Lp->pl0[p][es] : 0.0f;
                    clam[p][1] = 0.0f;
                    clam[p][2] = 0.0f;
                }
                if (RB > CGR && nxr > 0) load_xs(false);
                init_bounds();
                solve_w(IC<2>{}, IC<0>{}, mgi_c);
            }
