// The body of one NTT pass (csrc/ntt.hip includes it twice: `ntt_pass`, one butterfly per thread per stage, and `ntt_pass_r4`, two
// stages per sweep with four elements per thread).  Textual inclusion, not a function: the kernel's argument block is indexed
// dynamically (in_b[blockIdx.y], pre[tid]) and must stay in the kernel-argument segment -- handed to a helper by reference it
// is copied to scratch memory (1 KB per lane).  SG_NTT_R4 is 0 or 1.
  constexpr bool R4 = SG_NTT_R4 != 0;
  side_kernel_prio();
  extern __shared__ uint4 lds[];
  typedef Fr29 P;
  const fp_words* __restrict__ p_in = p.in_b[blockIdx.y];
  fp_words* __restrict__ p_out = p.out_b[blockIdx.y];
  const uint32_t R = 1u << p.log_r, T = 1u << p.log_t;
  const uint32_t E = R << p.log_t, H = (R >> 1) + 8;  // twiddles + 6 converted constants
  LdsTile d{lds, lds + E, reinterpret_cast<uint32_t*>(lds + 2 * E)};
  uint4* wbase = lds + 2 * E + ((E + 3) >> 2);
  LdsTile w{wbase, wbase + H, reinterpret_cast<uint32_t*>(wbase + 2 * H)};
  const uint32_t CONST0 = R >> 1;  // w-tile slots CONST0.. hold pre[0..2], post[0..2] in the 2^261 domain
  const uint32_t tid = threadIdx.x, nthr = blockDim.x;

  const uint32_t tiles_per_row = 1u << (p.log_b - p.log_t);
  const uint32_t a = blockIdx.x >> (p.log_b - p.log_t);  // outer index (Y only; 0 for X)
  const uint32_t b0 = (blockIdx.x & (tiles_per_row - 1)) << p.log_t;
  const size_t base = ((size_t)a << (p.log_b + p.log_r)) + b0;

  // stage the local twiddles (already 2^261-domain words) and convert the scale constants
  for (uint32_t k = tid; k < (R >> 1); k += nthr) lds_put(w, k, f29_load_r256<P>(p.tw_local + k));
  if (tid < 6 && ((tid < 3) ? p.pre3 : p.post3)) {
    const uint32_t* src = tid < 3 ? p.pre[tid] : p.post[tid - 3];
    uint32_t tmp[8];
#pragma unroll
    for (int i = 0; i < 8; i++) tmp[i] = src[i];
    f29 c = f29_words_to_r261<P>(tmp);
    if (tid >= 3 && p.fold29) {   // c * 2^232 * 2^-261 = c * 2^-29
      f29 k = f29_zero();
      k.l[8] = 1;
      c = f29_mul<P>(c, k);
    }
    lds_put(w, CONST0 + tid, c);
  }
  if (p.pre3) __syncthreads();
  // load the tile: rows are bit-reversed on the way in so that the DIT stages below leave
  // natural order
  const uint32_t rshift = 32 - p.log_r;
  if (p.skip) {
    // zero-padded input (coeff_to_extended: 2^k coefficients in a 2^(k+3) transform): only rows r < R >> skip exist,
    // they land on the positions that are multiples of 2^skip, and the first `skip` stages would only add zeros to
    // them -- u + w*0, u - w*0 -- i.e. copy each value over its block of 2^skip positions.  Load them replicated.
    const uint32_t keep = ~((1u << p.skip) - 1);
    for (uint32_t e = tid; e < E; e += nthr) {
      const uint32_t t = e & (T - 1), rr = e >> p.log_t;
      const uint32_t r = __brev(rr & keep) >> rshift;
      const size_t gi = base + t + ((size_t)r << p.log_b);
      f29 v = f29_load_r256<P>(p_in + gi);
      if (p.pre3) {
        uint32_t m = (uint32_t)(gi % 3);
        if (m) v = f29_mul<P>(v, lds_get(w, CONST0 + m));
      }
      lds_put(d, e, v);
    }
  } else {
  for (uint32_t e = tid; e < E; e += nthr) {
    uint32_t t = e & (T - 1), r = e >> p.log_t;
    size_t gi = base + t + ((size_t)r << p.log_b);
    f29 v;
    if (gi < p.in_len) {
      v = f29_load_r256<P>(p_in + gi);
      if (p.pre3) {
        uint32_t m = (uint32_t)(gi % 3);
        if (m) v = f29_mul<P>(v, lds_get(w, CONST0 + m));
      }
      if (p.pre_tab) v = f29_mul<P>(v, f29_load_r256<P>(p.pre_tab_b[blockIdx.y] + gi));   // x~ * (c^gi)^ = (x c^gi)~, bound < 2
    } else {
      v = f29_zero();
    }
    uint32_t rr = p.log_r ? (__brev(r) >> rshift) : 0;
    lds_put(d, (rr << p.log_t) + t, v);
  }
  }
  __syncthreads();

  // log2(R) radix-2 DIT stages, one butterfly per thread per sweep -- or (p.radix4) two stages per sweep: a thread takes the four
  // elements row, row + h, row + 2h, row + 3h of a 4h-block, runs the two butterflies of stage s and the two of stage s + 1 on
  // them in registers (the SAME operations on the same values in the same order: bit-identical tiles, the same bounds), and the
  // tile crosses LDS and a barrier once per two stages; the two butterflies of a stage are independent products.  An odd
  // number of stages starts with one radix-2 stage.
  auto butterfly = [&](f29& u, f29& v, uint32_t st, uint32_t j) {
    if (st < 2 && j == 0) {
      // w^0 butterflies of the first two stages skip the product (as best_fft does):
      // bounds 1 -> 3 (stage 0) and 3 -> 7 (stage 1)
      const f29 a = f29_add(u, v);
      v = st == 0 ? f29_sub<P, 0>(u, v) : f29_sub<P, 1>(u, v);
      u = a;
    } else {
      const f29 m = f29_mul<P>(v, lds_get(w, j << (p.log_r - st - 1)));  // bound(v) <= 25, twiddle canonical
      v = f29_sub<P, 0>(u, m);
      u = f29_add(u, m);
    }
  };
  uint32_t s = p.skip;
  const uint32_t single_end = R4 ? p.skip + ((p.log_r - p.skip) & 1u) : p.log_r;
  for (; s < single_end; s++) {
    const uint32_t h = 1u << s;
    for (uint32_t q = tid; q < (E >> 1); q += nthr) {
      uint32_t t = q & (T - 1), pr = q >> p.log_t;
      uint32_t j = pr & (h - 1), blk = pr >> s;
      uint32_t row = (blk << (s + 1)) + j;
      uint32_t i0 = (row << p.log_t) + t, i1 = i0 + (h << p.log_t);
      f29 u = lds_get(d, i0);
      f29 v = lds_get(d, i1);
      butterfly(u, v, s, j);
      lds_put(d, i0, u);
      lds_put(d, i1, v);
    }
    __syncthreads();
  }
  if constexpr (R4)
  for (; s < p.log_r; s += 2) {
    const uint32_t h = 1u << s, step = h << p.log_t;
    for (uint32_t q = tid; q < (E >> 2); q += nthr) {
      const uint32_t t = q & (T - 1), pr = q >> p.log_t;
      const uint32_t j = pr & (h - 1), blk = pr >> s;
      const uint32_t i0 = ((((blk << (s + 2)) + j)) << p.log_t) + t, i1 = i0 + step, i2 = i1 + step, i3 = i2 + step;
      f29 x0 = lds_get(d, i0), x1 = lds_get(d, i1), x2 = lds_get(d, i2), x3 = lds_get(d, i3);
      butterfly(x0, x1, s, j);
      butterfly(x2, x3, s, j);
      butterfly(x0, x2, s + 1, j);
      butterfly(x1, x3, s + 1, j + h);
      lds_put(d, i0, x0);
      lds_put(d, i1, x1);
      lds_put(d, i2, x2);
      lds_put(d, i3, x3);
    }
    __syncthreads();
  }

  // write back: one closing product per element (or, with nothing to multiply by, a product-free reduction), then the
  // canonical 32-byte store
  auto close_and_store = [&](f29 v, size_t go) {
    if (p.tw_pass) {
      v = f29_mul<P>(v, f29_load_r256<P>(p.tw_pass + go));
      if (p.post3) v = f29_mul<P>(v, lds_get(w, CONST0 + 3 + (uint32_t)(go % 3)));
    } else if (p.post3) {
      v = f29_mul<P>(v, lds_get(w, CONST0 + 3 + (uint32_t)(go % 3)));
    } else {
      v = p.fold29 ? f29_mont_step<P>(v) : f29_reduce_small<P>(v);
    }
    f29_store_canonical<P>(p_out + go, v);
  };
  if (p.kind == 0) {
    for (uint32_t e = tid; e < E; e += nthr) {
      uint32_t t = e & (T - 1), r = e >> p.log_t;
      close_and_store(lds_get(d, e), base + t + ((size_t)r << p.log_b));
    }
  } else {
    for (uint32_t e = tid; e < E; e += nthr) {
      uint32_t r = e & (R - 1), t = e >> p.log_r;
      uint32_t b = b0 + t;
      uint32_t bp = (b >> p.sig_lo) + ((b & ((1u << p.sig_lo) - 1)) << p.sig_hi);
      close_and_store(lds_get(d, (r << p.log_t) + t), ((size_t)bp << p.log_r) + r);
    }
  }
