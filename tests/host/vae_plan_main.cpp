// The VAE filter's planner on its own: csrc/p3d_vae_layout.h and nothing else, built by
// tests/test_vae_plan.py with the host compiler under AddressSanitizer and UBSan.
//
// stdin: one shape per line, "kind in n_enc enc.. latent n_dec dec.. out".  stdout: one line per
// shape, "status lds bones_or_elbo_lds dec_lds dec_staggered seq_lds P Ppk act nl nt dec_base
// seq_len seq_xoff seq_toff seq_ldt seq_moff ws64 npk" -- `status` -1 where vae_check_shape refuses
// (the rest then 0), else vae_plan's; ws64 the workspace floats at max_batch 64; npk the length of
// the flat-to-packed index, every entry of which is checked to lie inside the packed copy.
#include "../../3d-pose-baseline_amd/csrc/p3d_vae_layout.h"

#include <cstdio>

int main() {
  int kind, in, n_enc, n_dec, latent, out;
  int32_t enc[8], dec[8];
  while (scanf("%d %d %d", &kind, &in, &n_enc) == 3) {
    if (n_enc < 0 || n_enc > 8) return 2;
    for (int e = 0; e < n_enc; ++e)
      if (scanf("%d", &enc[e]) != 1) return 2;
    if (scanf("%d %d", &latent, &n_dec) != 2 || n_dec < 0 || n_dec > 8) return 2;
    for (int e = 0; e < n_dec; ++e)
      if (scanf("%d", &dec[e]) != 1) return 2;
    if (scanf("%d", &out) != 1) return 2;
    VaeShape s;
    VaePlan p;
    std::string err;
    if (vae_check_shape(kind, in, n_enc, enc, latent, n_dec, dec, out, s, err)) {
      printf("-1 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0\n");
      continue;
    }
    const int status = vae_plan(s, p, err);
    VaeShape other = s;   // the same widths as the other kind (a bones filter's out is 64)
    other.kind = kind == P3D_VAE_KIND_BONES ? P3D_VAE_KIND_ELBO : P3D_VAE_KIND_BONES;
    if (other.kind == P3D_VAE_KIND_BONES) other.out = 64;
    VaePlan q;
    std::string err2;
    (void)vae_plan(other, q, err2);
    const std::vector<int> idx = vae_pack_index(p.desc);
    for (int i : idx)
      if (i < 0 || i >= p.desc.Ppk) return 3;
    if ((int)p.names.size() != (int)p.tensors.size() || p.desc.nl > P3D_VAE_MAX_L || p.desc.nt > P3D_VAE_MAX_T) return 4;
    printf("%d %zu %zu %zu %zu %zu %d %d %d %d %d %d %d %d %d %d %d %lld %zu\n", status, p.lds, q.lds, p.dec_lds,
           vae_dec_bytes_staggered(s), p.seq_lds, p.desc.P, p.desc.Ppk, p.desc.act, p.desc.nl, p.desc.nt, p.dec_base,
           p.seq_len, p.seq_xoff, p.seq_toff, p.seq_ldt, p.seq_moff, (long long)p.ws_floats(64), idx.size());
  }
  return 0;
}
