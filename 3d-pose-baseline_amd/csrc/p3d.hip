// p3d.hip -- MI355X (gfx950) kernels and the C ABI (include/p3d.h) of the 2D->3D
// pose-lifting MLP: the hot path of EsauPR/3d-pose-baseline src/linear_model.py.
//
// Kernels (one launch each, all on the caller's stream):
//   k_fwd        Y = epi(X*W + b): fp32 MFMA GEMM on fragment-major operands + fused
//                epilogue (max-norm scale, bias, BN eval|train (+moving-average update),
//                ReLU, Philox dropout, residual add).     linear_model.py:103-124,171-199
//   k_dgrad      dX = dZ*W^T (+ residual grad) fused with the PREVIOUS layer's
//                dropout/ReLU/BN backward -> dZ_prev, dgamma, dbeta.
//   k_wgrad      dW = X^T*dZ and db = colsum(dZ) (64x64 tiles, LDS staged).
//   k_adam       TF1 ApplyAdam over the flat trainable buffer.  linear_model.py:137,145
//   k_pack       W (TF layout) -> the two fragment-major operand copies Wf / Wd.
//   k_mse        loss = mean((y-t)^2), dy = 2(y-t)/(B*D).     linear_model.py:129
//   k_mpjpe      fused un-normalize + per-joint L2 (fp64).   predict_3dpose.py:399-430
//   k_dot_*      per-tensor reductions for --max_norm (||W||^2, <G,W>).
#include <hip/hip_ext.h>
#include "p3d_kernels.h"
#include "p3d_bf16.h"
#include "p3d_eval.h"
#include "p3d_gemm.h"
#include "p3d_data.h"
#include "p3d_sample.h"
#include "p3d_clip.h"
#include "p3d_clips.h"
#include "p3d_live.h"
#include "p3d_skel.h"
#include "p3d_spline.h"
#include "p3d_traj.h"
#include "p3d_serve.h"
#include "p3d_serve6.h"
#include "p3d_serve_plan.h"
#include "p3d_gemv.h"
#include "p3d_xchg.h"
#include "../../include/p3d.h"

#include <math.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <cstdlib>
#include <mutex>
#include <string>
#include <unordered_set>
#include <vector>

#include "p3d_layers.h"
#include "p3d_vae.h"
#include "p3d_bones.h"
#include "p3d_vae_seq.h"
#include "p3d_vae_wide.h"
#include "p3d_vae_noise.h"
#include "p3d_vae_dec.h"
#include "p3d_vae_mc.h"

// The host side, one file per concern (each says in its header what it holds and stands on)
#include "p3d_host.h"
#include "p3d_model.h"
#include "p3d_forward_host.h"
#include "p3d_serve_host.h"
#include "p3d_train_host.h"
#include "p3d_data_host.h"
// The VAE pose filter, its noise and its bones (include/p3d.h; kernels in p3d_vae*.h, p3d_bones.h)
#include "p3d_vae_host.h"
// One clip, a batch of clips, live streams: p3d_clip_host.h also holds the stage the three share
#include "p3d_clip_host.h"
#include "p3d_clips_host.h"
#include "p3d_live_host.h"
// Lifted rows as a rigid skeleton: bone lengths, rotations, rigid pose (kernels in p3d_skel.h)
#include "p3d_skel_host.h"
// Spline-resampled clips: the fit, the samples and the lift over them (kernels in p3d_spline.h)
#include "p3d_spline_host.h"
// The root trajectory of lifted rows: the pinhole solve per frame and its windowed mean (kernels in p3d_traj.h)
#include "p3d_traj_host.h"

#include "p3d_dp.h"
