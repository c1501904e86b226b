// pybind11 bindings for the deep_go_amd HIP kernels (module `_dghip`).  dg_api.h declares every
// launcher (with its table layouts, optional pointers and preconditions); dg_bind.h says how
// they cross the boundary.
#include "dg_bind.h"

PYBIND11_MODULE(_dghip, m) {
  m.doc() = "deep_go_amd CDNA4 (gfx950) HIP kernels";
  m.attr("EPI_LINEAR") = 0;
  m.attr("EPI_FWD") = 1;
  m.attr("EPI_DGRAD") = 2;

  // conv_mfma.hip
  Bind<&dg_conv_nt>::def(m, "conv_nt");
  Bind<&dg_conv_nt_ex>::def(m, "conv_nt_ex", "conv_nt + optional ReLU bitmask output (EPI_FWD)");
  Bind<&dg_conv_wgrad>::def(m, "conv_wgrad");
  Bind<&dg_conv_wgrad_multi>::def(
      m, "conv_wgrad_multi", "weight gradients of several same-shape layers in one three-slice launch");
  Bind<&dg_conv_wgrad_set_ablate>::def(m, "conv_wgrad_set_ablate");
  Bind<&dg_conv_wgrad5_set_ns>::def(
      m, "conv_wgrad5_set_ns",
      "5x5 weight gradient: 0 = conv_wgrad_kernel, 4 | 5 = conv_wgrad_pipe_kernel stages");
  Bind<&dg_conv_wgrad_wgs_per_cu>::def(m, "conv_wgrad_wgs_per_cu");
  Bind<&dg_conv_wgrad_ktile>::def(m, "conv_wgrad_ktile");
  Bind<&dg_conv_wgrad_wgs_per_cu_for>::def(m, "conv_wgrad_wgs_per_cu_for");
  m.def("wgrad_reduce", [](uintptr_t slab, uintptr_t out, int splits, int M, int Mpad, int KP,
                           int taps, int cin, int cinp, uintptr_t bpart, int bchunks,
                           uintptr_t gposb, uintptr_t gbias, uintptr_t sf, uintptr_t stream) {
    check(dg_wgrad_reduce(P<float>(slab), P<float>(out), splits, M, Mpad, KP, taps, cin, cinp,
                          P<float>(bpart), bchunks, P<float>(gposb), P<float>(gbias), nullptr,
                          nullptr, nullptr, P<long long>(sf), S(stream)),
          "wgrad_reduce");
  });
  Bind<&dg_wgrad_reduce>::def(
      m, "wgrad_reduce_w",
      "wgrad_reduce writing bf16 twins of the weight / position-bias / bias gradients too");
  m.def("wgrad_reduce_multi", [](uintptr_t table, int nl, uintptr_t stream) {
    check(dg_wgrad_reduce_multi(P<long long>(table), nl, 13, S(stream)), "wgrad_reduce_multi");
  }, "slab reduce + bias pass 2 of nl layers in one launch (13-column table rows)");
  m.def("wgrad_reduce_multi_w", [](uintptr_t table, int nl, uintptr_t stream) {
    check(dg_wgrad_reduce_multi(P<long long>(table), nl, 16, S(stream)), "wgrad_reduce_multi_w");
  }, "wgrad_reduce_multi writing bf16 twins too (16-column table rows)");

  // conv_board.hip
  Bind<&dg_conv_board>::def(m, "conv_board");
  Bind<&dg_conv_board_ex>::def(
      m, "conv_board_ex",
      "conv_board + optional bf16 bias table (fwd) and ReLU bitmask (fwd writes, dgrad reads)");
  Bind<&dg_conv_board_set_ablate>::def(
      m, "conv_board_set_ablate", "diagnostics: 1 skip MFMA, 2 skip LDS fragment reads, 4 skip DMA");

  // conv_stack2.hip: weights streamed into VGPRs (fragment-ordered), no per-K-step barrier
  m.def("conv_stack2_fwd", [](uintptr_t table, int nl, uintptr_t X0, int l1, int B,
                              uintptr_t stream) {
    check(dg_conv_stack2(1, P<long long>(table), nl, P<void>(X0), l1, B, S(stream)),
          "conv_stack2_fwd");
  }, "conv_stack2 forward; l1: table row 0 = the network's first layer");
  Bind<&dg_conv_stack2>::def(
      m, "conv_stack2",
      "conv_stack2: EPI_FWD forward or EPI_DGRAD backward-data chain (fragment-ordered A)");
  Bind<&dg_conv_stack2_fwd_head>::def(m, "conv_stack2_fwd_head",
                                      "conv_stack2 forward + the fused 3x3/128 policy head");
  Bind<&dg_conv_stack2_fwd_head_x>::def(
      m, "conv_stack2_fwd_head_x",
      "conv_stack2 forward (l1) with the feature expansion fused into its prologue + the head");
  Bind<&dg_conv_stack2_set_mode>::def(
      m, "conv_stack2_set_mode",
      "conv_stack2 timing-ablation mode (tools/kbench_stack.py; 0 = production)");
  Bind<&dg_conv_stack2_set_sched>::def(
      m, "conv_stack2_set_sched",
      "conv_stack2 schedule: staggered two-group on / off (overrides DG_STACK2_STAG), co-half-0 "
      "MFMA priority 0..2, co-half-1 start delay");

  // conv_layer2.hip
  Bind<&dg_conv_layer2>::def(
      m, "conv_layer2",
      "one hidden 3x3 C -> C layer (C = 256 | 128) on conv_stack2's K loop: epi 1 forward "
      "(fragment weights, pbias_frag, mask written), 2 backward-data (mask of the layer below)");
  Bind<&dg_conv_layer2_multi>::def(
      m, "conv_layer2_multi", "a run of nl conv_layer2 layers in one launch");
  Bind<&dg_conv_layer2_multi_head>::def(
      m, "conv_layer2_multi_head",
      "d = 256 forward run + the fused 3x3/256 policy head on its last output");

  // conv_stack_f8.hip: the fp8 (MX MFMA) stack of the hidden C -> C layers
  m.def("conv_stack_f8", [](int C, int epi, uintptr_t table, int nl, uintptr_t X0,
                            uintptr_t s_x0, uintptr_t amax_x0, int B, uintptr_t stream) {
    check(dg_conv_stack_f8(C, epi, P<long long>(table), nl, P<void>(X0), P<float>(s_x0),
                           P<unsigned>(amax_x0), B, nullptr, nullptr, S(stream)),
          "conv_stack_f8");
  }, "fp8 layer stack (C = 128 | 256; epi 1 forward e4m3, 2 backward-data e5m2)");
  m.def("conv_stack_f8_y8", [](int C, int epi, uintptr_t table, int nl, uintptr_t X0,
                               uintptr_t s_x0, uintptr_t amax_x0, int B, uintptr_t y8,
                               uintptr_t stream) {
    check(dg_conv_stack_f8(C, epi, P<long long>(table), nl, P<void>(X0), P<float>(s_x0),
                           P<unsigned>(amax_x0), B, P<long long>(y8), nullptr, S(stream)),
          "conv_stack_f8_y8");
  }, "conv_stack_f8 + fp8 copy-out (the y8 list)");
  m.def("conv_stack_f8_dgrad", [](int C, uintptr_t table, int nl, uintptr_t X0,
                                  uintptr_t s_x0, uintptr_t amax_x0, int B, uintptr_t y8,
                                  uintptr_t sr_step, uintptr_t stream) {
    check(dg_conv_stack_f8(C, 2, P<long long>(table), nl, P<void>(X0), P<float>(s_x0),
                           P<unsigned>(amax_x0), B, P<long long>(y8), P<long long>(sr_step),
                           S(stream)),
          "conv_stack_f8_dgrad");
  }, "the e5m2 backward-data stack (conv_stack_f8 epi 2) with optional fp8 copies (y8, 0: "
     "none) and stochastic rounding seeded by the int64 device step counter sr_step (0: "
     "round to nearest even)");
  m.def("conv_stack_f8_fwd_head", [](int C, uintptr_t table, int nl, uintptr_t X0,
                                     uintptr_t s_x0, uintptr_t amax_x0, int B, uintptr_t w,
                                     uintptr_t bias, uintptr_t posb, uintptr_t labels,
                                     uintptr_t loss, uintptr_t pred, uintptr_t dZ,
                                     uintptr_t gw_part, uintptr_t dzb, int head_relu,
                                     float grad_scale, uintptr_t stream) {
    check(dg_conv_stack_f8_fwd_head(C, P<long long>(table), nl, P<void>(X0), P<float>(s_x0),
                                    P<unsigned>(amax_x0), B, P<float>(w), P<float>(bias),
                                    P<float>(posb), P<int>(labels), P<float>(loss), P<int>(pred),
                                    P<void>(dZ), P<float>(gw_part), P<float>(dzb), head_relu,
                                    grad_scale, nullptr, S(stream)),
          "conv_stack_f8_fwd_head");
  }, "fp8 forward stack + the fused 3x3 policy head (C = 128 | 256)");
  Bind<&dg_conv_stack_f8_fwd_head>::def(
      m, "conv_stack_f8_fwd_head_y8",
      "conv_stack_f8_fwd_head + fp8 copy-out (y8 as conv_stack_f8_y8)");
  Bind<&dg_conv_stack_f8_set_mode>::def(m, "conv_stack_f8_set_mode",
                                        "conv_stack_f8 timing-ablation mode (0 = production)");
  Bind<&dg_conv_stack_f8_set_debug>::def(
      m, "conv_stack_f8_set_debug",
      "conv_stack_f8 diagnostics: s_memtime phase stamps of boards 0..7 into dbg (0 = off)");
  Bind<&dg_conv_stack_f8_set_sched>::def(
      m, "conv_stack_f8_set_sched",
      "conv_stack_f8 (C = 128) schedule: staggered two-group on / off (overrides "
      "DG_STACK_F8_STAG; 0 off, 1 both stacks, 2 backward-data only), co-half-1 start delay");

  // conv_wgrad_win.hip, conv_wgrad_win8.hip
  Bind<&dg_conv_wgrad_win>::def(
      m, "conv_wgrad_win",
      "sliding-window 3x3 weight gradients (frame-linear K, 9 taps per staged X window)");
  Bind<&dg_conv_wgrad_win_splits>::def(m, "conv_wgrad_win_splits");
  Bind<&dg_conv_wgrad_win_set_ablate>::def(m, "conv_wgrad_win_set_ablate");
  Bind<&dg_conv_wgrad_win8>::def(m, "conv_wgrad_win8",
                                 "MX-fp8 sliding-window weight gradients (448-row fp8 frames)");
  Bind<&dg_conv_wgrad_win8_splits>::def(m, "conv_wgrad_win8_splits");
  Bind<&dg_conv_wgrad_win8_set_ablate>::def(
      m, "conv_wgrad_win8_set_ablate",
      "conv_wgrad_win8 timing ablation (tools/kbench_win8.py; 0 = production): 1 no MFMA, "
      "2 no LDS reads, 4 no LDS-DMA, 8 no slab store, 16 no barrier (sums of these)");

  // conv_l1.hip
  Bind<&dg_conv_l1>::def(
      m, "conv_l1",
      "board-resident first-layer forward (conv_l1.hip): bias + position bias (fp32, or the "
      "bf16 pbias table when given) + ReLU");
  Bind<&dg_conv_l1_ok>::def(m, "conv_l1_ok");
  Bind<&dg_conv_l1_frag>::def(
      m, "conv_l1_frag",
      "5x5 / 40-channel first layer, one board per workgroup, fragment-ordered weights "
      "(conv_l1.hip conv_l1_frag_kernel); planes/player/rank non-zero: the feature expansion "
      "fused in (X written)");
  Bind<&dg_conv_l1_frag_ok>::def(m, "conv_l1_frag_ok");

  // conv_fp8.hip
  Bind<&dg_conv_board_fp8>::def(m, "conv_board_fp8");
  Bind<&dg_fp8_update_scales>::def(m, "fp8_update_scales");
  Bind<&dg_weight_fp8>::def(m, "weight_fp8");
  Bind<&dg_frame_to_fp8>::def(m, "frame_to_fp8");

  // head.hip
  m.def("head_reduce", [](uintptr_t dzb, uintptr_t gw_part, int B, int n, uintptr_t gw,
                          uintptr_t gbias, uintptr_t gposb, uintptr_t sf, uintptr_t stream) {
    check(dg_head_reduce(P<float>(dzb), P<float>(gw_part), B, n, P<float>(gw), P<float>(gbias),
                         P<float>(gposb), nullptr, nullptr, nullptr, P<long long>(sf), S(stream)),
          "head_reduce");
  });
  Bind<&dg_head_reduce>::def(m, "head_reduce_w", "head_reduce writing bf16 twins too");
  Bind<&dg_head>::def(m, "head");

  // elementwise.hip
  m.def("expand_features", [](uintptr_t planes, uintptr_t player, uintptr_t rank, uintptr_t out,
                              int B, int pad, int CP, uintptr_t stream) {
    check(dg_expand_features(P<uint8_t>(planes), P<uint8_t>(player), P<uint8_t>(rank),
                             P<void>(out), B, pad, CP, nullptr, 0, S(stream)),
          "expand_features");
  });
  Bind<&dg_bias_grad_partial>::def(m, "bias_grad_partial");
  Bind<&dg_bias_grad_partial_multi>::def(m, "bias_grad_partial_multi");
  Bind<&dg_bias_chunks>::def(m, "bias_chunks");
  Bind<&dg_bias_chunks_multi>::def(m, "bias_chunks_multi");
  m.def("sgd", [](uintptr_t p, uintptr_t g, size_t n, uintptr_t lr, float gscale,
                  uintptr_t gate, uintptr_t stream) {
    check(dg_sgd(P<float>(p), P<float>(g), n, P<double>(lr), gscale, P<float>(gate), nullptr,
                 S(stream)),
          "sgd");
  });
  m.def("sgd_bf16", [](uintptr_t p, uintptr_t g16, size_t n, uintptr_t lr, float gscale,
                       uintptr_t gate, uintptr_t stream) {
    check(dg_sgd(P<float>(p), nullptr, n, P<double>(lr), gscale, P<float>(gate), P<void>(g16),
                 S(stream)),
          "sgd_bf16");
  }, "SGD reading the bf16 (wire-format) gradient");
  m.def("rmsprop", [](uintptr_t p, uintptr_t g, uintptr_t ms, size_t n, uintptr_t lr,
                      float decay, float gscale, uintptr_t gate, uintptr_t stream) {
    check(dg_rmsprop(P<float>(p), P<float>(g), P<float>(ms), n, P<double>(lr), decay, gscale,
                     P<float>(gate), nullptr, S(stream)),
          "rmsprop");
  });
  m.def("rmsprop_bf16", [](uintptr_t p, uintptr_t g16, uintptr_t ms, size_t n, uintptr_t lr,
                           float decay, float gscale, uintptr_t gate, uintptr_t stream) {
    check(dg_rmsprop(P<float>(p), nullptr, P<float>(ms), n, P<double>(lr), decay, gscale,
                     P<float>(gate), P<void>(g16), S(stream)),
          "rmsprop_bf16");
  }, "RMSProp reading the bf16 (wire-format) gradient");
  m.def("finite_gate", [](uintptr_t loss, int n, uintptr_t grads, size_t ng, uintptr_t gate,
                          uintptr_t bad, uintptr_t stream) {
    check(dg_finite_gate(P<float>(loss), n, P<float>(grads), ng, P<float>(gate), P<int>(bad),
                         nullptr, S(stream)),
          "finite_gate");
  });
  m.def("finite_gate_bf16", [](uintptr_t loss, int n, uintptr_t grads16, size_t ng,
                               uintptr_t gate, uintptr_t bad, uintptr_t stream) {
    check(dg_finite_gate(P<float>(loss), n, nullptr, ng, P<float>(gate), P<int>(bad),
                         P<void>(grads16), S(stream)),
          "finite_gate_bf16");
  }, "finite_gate over the bf16 (wire-format) gradient");
  Bind<&dg_finite_gate1>::def(
      m, "finite_gate1",
      "loss + gradient finite gate in one launch (fp32 grads or the bf16 twin grads16)");
  Bind<&dg_lr_decay>::def(m, "lr_decay");
  m.def("weight_refresh", [](uintptr_t table, int n, uintptr_t stream) {
    check(dg_weight_refresh(P<long long>(table), n, nullptr, 0.0, nullptr, S(stream)),
          "weight_refresh");
  });
  Bind<&dg_weight_refresh>::def(m, "weight_refresh_decay");
  Bind<&dg_grad_update_cols>::def(m, "grad_update_cols");
  Bind<&dg_grad_update_tickets>::def(
      m, "grad_update_tickets",
      "uint32 ticket counters grad_update needs (zeroed once; the kernel leaves them zeroed)");
  Bind<&dg_grad_update>::def(
      m, "grad_update",
      "fused gradient pass 2 (slabs / bias partials, or the flat gradient) + SGD / RMSProp + "
      "operand refresh + LR decay (elementwise.hip grad_update_kernel)");
  Bind<&dg_comm_proxy>::def(m, "comm_proxy");

  // policy.hip
  Bind<&dg_symmetry_planes>::def(
      m, "symmetry_planes",
      "boards i S + s of a packed batch of capacity B <- source board i moved by symmetry s "
      "(policy.hip)");
  Bind<&dg_policy_ensemble>::def(
      m, "policy_ensemble",
      "symmetry-averaged, legality-masked policy with top-k and label rank (policy.hip)");
}
