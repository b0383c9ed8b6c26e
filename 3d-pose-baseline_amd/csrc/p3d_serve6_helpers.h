// p3d_serve6_helpers.h -- the rounds form with helper waves: the loop of rounds of a 512-thread
// k_serve6_rounds, included as text by p3d_serve6_body.h where HELPERS is set (PAIR and ROUNDS are).
// (No include guard: one inclusion per kernel.)
//
// Two waves per SIMD.  Waves 0-3 contract: wave w keeps its K slice and the register ring, which
// runs on from block to block, and between two contractions does nothing but write its accumulators
// to red[s & 1] and count on an LDS word.  Waves 4-7 finish: wave 4 + w does what wave w of the
// 256-thread form does between contractions -- K-combine, epilogue, stores, the post, the next
// round's input layers, the previous round's output tiles, the closing output phase -- with the
// same tile dealing (u = w + 4 j), the same slice order and the same clamped duplicates: every bit
// as in the 256-thread form.  Three LDS words tie the roles together:
//   sh[7]  partials written: each contraction wave adds 1 behind its LDS writes of block q (4 per
//          block); the helpers read red[q & 1] once it stands at 4 (q + 1);
//   sh[8]  partials read: each helper wave adds 1 once its LDS reads of block q have returned (an odd
//          block whose boundary runs output tiles: once those are done, they use red[1]); a
//          contraction wave writes block q's partials only when it stands at 4 (q - 1), i.e. block
//          q - 2 is read -- two blocks back, so the check does not wait in a healthy launch;
//   sh[9]  the helpers' own barrier (hbar).
// No s_barrier inside the loop: the contraction waves never wait for the helpers.
//
// Posts.  A helper wave posts block q right behind its stores (s_waitcnt vmcnt(0), post_wave: the
// fourth helper stores the member's flag), so flag value q + 3 publishes block q, the value the
// 256-thread form posts from inside block q + 1's contraction; a contraction wave counts the same
// numbers without posting and checks, as before, value q + 2 before block q's tail requests block
// q + 1's operands.  A helper's order per block: the next round's input layer (blocks 2 NH - 2 and
// 2 NH - 1, while the block contracts), the wait for the partials, epilogue stores, then the post,
// which publishes both.  The previous round's output tiles run at block 1: in a
// one-block model (NH = 2) in front of that block's post, so that a member's post of block 1 says its
// output tiles are read -- the epilogue of block 2 NH - 2 = 2, which rewrites slab 3, is the unit's
// very next block, and its writer has seen every member's post of block 1 and no later one.  With
// NH >= 4 they run behind the post (nobody waits for them) and the post of block 2 covers them.
  const bool helper = __builtin_amdgcn_readfirstlane(tid >> 8) != 0;
  int qb = 0;                                // blocks this wave has handled (both roles count alike)
  // priority (MEASUREMENTS 22).  Static, once in front of the loops behind a wave-uniform branch: 1
  // raises the contraction waves, 2 the helper waves -- at equal priority the older contraction
  // wave's MFMA stream leaves the helper's few MFMAs (input layers, output tiles) no slot, and their
  // posts come late.
#if P3D_S6_HELPER_PRIO == 1
  if (!helper) __builtin_amdgcn_s_setprio(1);
#elif P3D_S6_HELPER_PRIO == 2
  if (helper) __builtin_amdgcn_s_setprio(1);
#endif

  // a bounded wait for an LDS counter (relaxed, workgroup scope; the partner role's LDS traffic is
  // ordered by its s_waitcnt in front of its add)
  auto lds_wait = [&](int* word, int target, int nap) {
    for (int spin = 0;; ++spin) {
      const int v = __builtin_amdgcn_readfirstlane(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
      if (v >= target) break;
      if (spin > P3D_SERVE_SPIN) {
        broken = true;
        sh[4] = 1;
        if (lane == 0) __hip_atomic_store(p.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        break;
      }
      if (nap) __builtin_amdgcn_s_sleep(P3D_S6_HELPER_NAP);
    }
    asm volatile("" ::: "memory");
  };
  // The helpers' input layer of the unit at rbase (this member's tiles, this wave's share u = w + 4 j).
  // in_issue / in_compute hold four k-groups of both operands of all UMAX tiles, 96 registers that the
  // one allocation of both roles does not have (they spilled 46): here the first two k-groups -- all of
  // K0 <= 32, the reference's 16 joints x 2 -- of every tile are requested at once, and the other two
  // (K0 in (32, 64]) per tile behind them.  Each tile's MFMA chain (k-groups in order), constants and
  // epilogue are in_compute's: the same bits.
  auto in_layer_h = [&](int64_t rbase, float* dst) {
    f32x4 xa[UMAX][2], wb[UMAX][2];
    const float* xr[UMAX];
    const float* wr[UMAX];
#pragma unroll
    for (int j = 0; j < UMAX; ++j) {
      const int u = min(w + 4 * j, RT * NCM - 1), rt = u / NCM, cc = u % NCM;
      int64_t rowc = rbase + 16 * rt + (lane & 15);
      rowc = rowc < p.M ? rowc : p.M - 1;
      const int t = t_lo + (cc < nck ? cc : nck - 1);
      xr[j] = p.x + rowc * p.K0 + q4;
      wr[j] = li.Wf + ((int64_t)t * ngK0 * 64 + lane) * 4;
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const int gg = min(g, ngK0 - 1);       // (g >= ngK0: a copy of the last k-group, never used)
        xa[j][g] = *(const f32x4*)(xr[j] + 16 * gg);
        wb[j][g] = *(const f32x4*)(wr[j] + gg * 256);
      }
    }
#pragma unroll
    for (int j = 0; j < UMAX; ++j) {
      const int u = w + 4 * j, rt = u / NCM, cc = u % NCM;
      if (u >= RT * NCM || cc >= nck) continue;
      const int t = t_lo + cc;
      const float* e = ec + (0 * ECT + (t - t_lo)) * 48 + q4;
      const f32x4 c0 = *(const f32x4*)e, c1 = *(const f32x4*)(e + 16), c2 = *(const f32x4*)(e + 32);
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int g = 0; g < 2; ++g)
        if (g < ngK0)
#pragma unroll
          for (int k = 0; k < 4; ++k) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[j][g][k], xa[j][g][k], acc, 0, 0, 0);
      if (ngK0 > 2) {                          // (one uniform branch for K0 in (32, 64])
        f32x4 xh[2], wh[2];
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          const int gg = min(2 + g, ngK0 - 1);
          xh[g] = *(const f32x4*)(xr[j] + 16 * gg);
          wh[g] = *(const f32x4*)(wr[j] + gg * 256);
        }
#pragma unroll
        for (int g = 0; g < 2; ++g)
          if (2 + g < ngK0)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wh[g][k], xh[g][k], acc, 0, 0, 0);
      }
      if (wsq_any) maxnorm_div(0, acc);
      *(f32x4*)(dst + ((int64_t)(rt * ngL + t) * 64 + lane) * 4) = epi_c(c0, c1, c2, acc);
    }
  };
  // ---- the group's first round: the helpers' input layers, A's posted by all eight waves' group_sync (which binds
  // the bank), B's by the helpers' own post; the contraction waves fill the ring meanwhile
  if (gi < p.nb) {
    const int64_t rowA = (int64_t)gi * ROWS, rowB = (int64_t)(gi + ng) * ROWS;
    if (helper) in_layer_h(rowA, act);
    group_sync(false, false);
    if (helper) {
      in_layer_h(rowB, act + 4 * slab);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      post_wave();                           // (value 2: block 1's producers)
    } else {
      wait_for(nsync);                       // A's input layer from this wave's K-slice producers
      P3D_S6_STAMP(trs, 3);
      const float *A0, *r0;
      float* Y0;
      slabs(0, 0, A0, Y0, r0);
      ring_load(1, A0);
    }
  }
  // (one loop of rounds per role: with the role chosen inside one loop the ring stayed live through
  // the helpers' path and the kernel spilled 294 registers)
  if (!helper) {
    // ---- contraction waves: block after block, the ring refilled across the boundary -------------
    for (int b = gi; b < p.nb; b += 2 * ng) {
      const bool has_next = b + 2 * ng < p.nb;
      const int rotn = (rot + 2 * p.nblk) % 3;
      for (int s = 0; s < 2 * NH; ++s) {
        const int ph = (s >> 1) + 1;
        const ServeLayer& ly = p.ly[ph];
        const float *A, *res;
        float* Y;
        slabs(s, rot, A, Y, res);
        const __amdgpu_buffer_rsrc_t ra = p3d_rsrc(A), rw = p3d_rsrc(ly.Wf);
        P3D_S6_STAMP(trs, 8 + 4 * s);
        P3D_S6_STAMP(rnd == 1 && s < 3, 41 + 8 * s);
        f32x4 acc[NCM][RT];
#pragma unroll
        for (int cc = 0; cc < NCM; ++cc)
#pragma unroll
          for (int t = 0; t < RT; ++t) acc[cc][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        auto mfmas = [&](int d) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int cc = 0; cc < NCM; ++cc)
#pragma unroll
              for (int t = 0; t < RT; ++t)
                acc[cc][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(rb_[d][cc][e], ra_[d][t][e], acc[cc][t], 0, 0, 0);
        };
        constexpr int kSlotLoads = RT + NCM;
        auto refill = [&](int d, const __amdgpu_buffer_rsrc_t& ra2, const __amdgpu_buffer_rsrc_t& rw2, int g) {
#pragma unroll
          for (int t = 0; t < RT; ++t) ra_[d][t] = p3d_ld_sc1(ra2, aoff0 + t * rstride + g * 1024);
#pragma unroll
          for (int cc = 0; cc < NCM; ++cc)
            rb_[d][cc] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rw2, voff, toff[cc] + g * 1024, 0));
        };
        auto round = [&](int g0) {
#pragma unroll
          for (int d = 0; d < DEPTH; ++d) {
            mfmas(d);
            refill(d, ra, rw, g0 + DEPTH + d);
            __builtin_amdgcn_sched_barrier(0);
          }
        };
        round(0);
        // These waves store nothing, so there is no post here and this wait publishes nothing: it only
        // marks, as in the 256-thread form, that the round's DEPTH (RT + NCM) refills are the youngest
        // requests in flight (everything older -- the previous tail's refills, the flag word -- was
        // consumed above), for the disassembly check of tests/test_serve_rounds_resources.py.
        asm volatile("s_waitcnt vmcnt(%0)\n\ts_nop 5" ::"n"(DEPTH * kSlotLoads) : "memory");
        ++nsync;                               // (the value the helpers post for the previous block)
        __builtin_amdgcn_sched_barrier(0);
        for (int g0 = DEPTH; g0 < gcount - 2 * DEPTH; g0 += DEPTH) round(g0);
        // the next block's producers: flags requested a round ahead of the check; and the helpers'
        // "read" word, for this block's partials
        const unsigned fl = __hip_atomic_load(flags + m0 + min(lane, cntw - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int rdw = __hip_atomic_load(&sh[8], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __builtin_amdgcn_sched_barrier(0);
        round(gcount - 2 * DEPTH);
        if (!broken) {
          if (__any(fl & 0x80000000u)) broken = true;
          else if (!__all((fl & 0x7fffffffu) >= nsync)) wait_for(nsync);
        }
        asm volatile("" ::: "memory");         // (as in the 256-thread form: the next operands behind the check)
        {
          const bool wrap = has_next && s == 2 * NH - 1;
          const int sn = wrap ? 0 : min(s + 1, 2 * NH - 1);
          const float *An, *rn;
          float* Yn;
          slabs(sn, wrap ? rotn : rot, An, Yn, rn);
          const __amdgpu_buffer_rsrc_t ran = p3d_rsrc(An), rwn = p3d_rsrc(p.ly[(sn >> 1) + 1].Wf);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int d = 0; d < DEPTH; ++d) {
            mfmas(d);
            refill(d, ran, rwn, d);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        P3D_S6_STAMP(trs, 8 + 4 * s + 1);
        P3D_S6_STAMP(rnd == 1 && s < 3, 42 + 8 * s);
        // the helpers have read block qb - 2 out of this buffer (two blocks back: no wait in a healthy
        // launch -- the word was read a ring round ago)
        if (__builtin_amdgcn_readfirstlane(rdw) < 4 * (qb - 1)) lds_wait(&sh[8], 4 * (qb - 1), 0);
        f32x4* rd = red + (s & 1) * (4 * RT * NCM * 64);
#pragma unroll
        for (int cc = 0; cc < NCM; ++cc)
#pragma unroll
          for (int t = 0; t < RT; ++t) rd[((w * RT + t) * NCM + cc) * 64 + lane] = acc[cc][t];
        if (broken) sh[4] = 1;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_fetch_add(&sh[7], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        ++qb;
      }
#ifdef P3D_TRACE
      if (trs && tr6 && tid == 0) tr6[8 * (NH + 1)] = wall_clock64();
      if (tid == 0 && blockIdx.x < 1024) g_p3d_trace[20480 + blockIdx.x] = wall_clock64();   // every member's end
      ++rnd;
#endif
      trs = false;
      rot = rotn;
    }
  } else {
    // ---- helper waves: every block's boundary work, off the contraction waves ---------------------
    for (int b = gi; b < p.nb; b += 2 * ng) {
      const int64_t rowA = (int64_t)b * ROWS, rowB = (int64_t)(b + ng) * ROWS;
      const bool has_next = b + 2 * ng < p.nb;
      const int rotn = (rot + 2 * p.nblk) % 3;
      f32x4 part[UMAX][4], ce[UMAX][3], rv[UMAX];
      for (int s = 0; s < 2 * NH; ++s) {
        const int php = (s >> 1) + 1;
        const float *Ap, *resp;
        float* Yp;
        slabs(s, rot, Ap, Yp, resp);
        // 1. the residual fragments, early: this member's own tiles, stored by this wave four blocks
        // ago (from A where there is no residual, unused): no other member's data, no flag to check
        const __amdgpu_buffer_rsrc_t rr = p3d_rsrc(resp ? resp : Ap);
#pragma unroll
        for (int j = 0; j < UMAX; ++j) {
          const int u = min(w + 4 * j, RT * NCM - 1), rt = u / NCM, cc = u % NCM;
          const int t = t_lo + (cc < nck ? cc : nck - 1);
          rv[j] = p3d_ld_sc1(rr, (int)(((int64_t)(rt * ngL + t) * 64 + lane) * 16));
        }
        // 6. a round's last two blocks: the next round's input layer of this block's unit, into slab
        // rotn of the unit -- while the block contracts, not behind it: it needs nothing of the block,
        // and behind the epilogue its post came so close to the other members' flag request (half a
        // contraction on) that their check fell to the polling path, 2-4 us per input layer.  Slab rotn
        // was last read in the unit's phase NH - 2, four blocks back: this wave finished block s - 1,
        // whose partials this member's contraction waves wrote after finding every member's post of
        // block s - 2, i.e. every member's contraction s - 2 done.  Published by this block's post.
        if (has_next && s >= 2 * NH - 2)
          in_layer_h(((s & 1) ? rowB : rowA) + (int64_t)2 * ng * ROWS, act + ((s & 1) * 4 + rotn) * slab);
        // 2. all four contraction waves have written block qb's partials
        lds_wait(&sh[7], 4 * (qb + 1), 1);
        broken = broken || sh[4] != 0;
        // 3. the K slices and the tiles' constants (red buffer s & 1), exactly as epi_rd / epi_st of the
        // 256-thread form
        {
          const f32x4* rdp = red + (s & 1) * (4 * RT * NCM * 64);
#pragma unroll
          for (int j = 0; j < UMAX; ++j) {
            const int u = min(w + 4 * j, RT * NCM - 1), rt = u / NCM, cc = u % NCM;
#pragma unroll
            for (int k = 0; k < 4; ++k) part[j][k] = rdp[((k * RT + rt) * NCM + cc) * 64 + lane];
            const int t = t_lo + (cc < nck ? cc : nck - 1);
            const float* e = ec + (php * ECT + (t - t_lo)) * 48 + q4;
#pragma unroll
            for (int k = 0; k < 3; ++k) ce[j][k] = *(const f32x4*)(e + 16 * k);
          }
        }
        // 4. the reads have returned: the buffer is the contraction waves' again -- but for an odd block
        // whose boundary runs output tiles, which keep red[1] until they are done
        const bool outs = b != gi && s == 1;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (!outs && lane == 0) __hip_atomic_fetch_add(&sh[8], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        {
          f32x4 sacc[UMAX];
#pragma unroll
          for (int j = 0; j < UMAX; ++j) {
            sacc[j] = part[j][0];              // slice 0, tile (rt, cc), then 1, 2, 3
#pragma unroll
            for (int k = 1; k < 4; ++k) sacc[j] += part[j][k];
          }
          if (wsq_any)
#pragma unroll
            for (int j = 0; j < UMAX; ++j) maxnorm_div(php, sacc[j]);
#pragma unroll
          for (int j = 0; j < UMAX; ++j) {
            // (a clamped duplicate where the wave or the member has fewer tiles: the same bits)
            const int u = min(w + 4 * j, RT * NCM - 1), rt = u / NCM, cc = u % NCM;
            const int t = t_lo + (cc < nck ? cc : nck - 1);
            f32x4 yv = epi_c(ce[j][0], ce[j][1], ce[j][2], sacc[j]);
            if (resp) yv += rv[j];
            *(f32x4*)(Yp + ((int64_t)(rt * ngL + t) * 64 + lane) * 4) = yv;
          }
        }
        // 7. the previous round's output tiles: its last hidden layers (slabs 3 / 7) were posted with
        // its last two blocks -- the later one a post before this wave's last (its own flag check:
        // this wave's K-slice producers).  In front of this block's post: see the head of this file.
        // With four or more blocks per unit (NH >= 4) the post goes first -- block 3 of every member
        // waits for it -- and the output tiles are covered by this wave's post of block 2 instead: slab
        // 3 is rewritten at block 2 NH - 2 >= 6, whose writer has seen every member post block 2 NH - 3.
        const bool post_first = outs && NH >= 4;
        if (post_first) {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          post_wave();
        }
        if (outs) {
          wait_for(nsync - (post_first ? 2 : 1));
          hbar();                              // every helper has read block 1's partials: red[1] is free
          out_phase(orowA, orowB, false);
          if (lane == 0) __hip_atomic_fetch_add(&sh[8], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        // 5. the post, behind every store of this boundary
        if (!post_first) {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          post_wave();
        }
        ++qb;
      }
      rot = rotn;
      orowA = rowA;
      orowB = rowB;
    }
    // ---- the group's last round: its output tiles (the last block's post is made) ----------------
    if (gi < p.nb) {
      wait_for(nsync);                       // both units' last hidden layers (slabs 3, 7)
      hbar();                                // (the last block is odd: every helper has read red[1])
      out_phase(orowA, orowB, false);
    }
  }
