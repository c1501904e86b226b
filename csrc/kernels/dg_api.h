// The C interface of the deep_go_amd HIP kernel library: every extern "C" dg_* host entry
// point, declared once.  Each .hip file includes this header, so its definitions are compiled
// against these declarations (a conflicting redeclaration of a C function is a compile
// error), and bindings.cpp derives the Python bindings from them.  Host-clean: no device code.
//
// Conventions: pointers are device addresses unless stated otherwise; a launch "table" is a
// HOST array of int64 rows (pointers and integers) read before the launch returns; "optional"
// pointers may be null.  Launchers validate the invariants they rely on and return
// hipErrorInvalidValue before touching the GPU.  epi: 0 linear, 1 forward (bias + position
// bias + ReLU), 2 backward-data (ReLU gate of the layer below).  sf: the int64 bad-step flag
// (optional), set when a reduced gradient leaves the accepted range.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

extern "C" {

// ---------------------------------------------------------------- conv_mfma.hip
// Conv (forward / dgrad / linear) via the NT implicit-GEMM kernel; mask (optional, EPI_FWD):
// the ReLU bitmask output.  dg_conv_nt = dg_conv_nt_ex without a mask.
hipError_t dg_conv_nt_ex(int epi, int kw, int bm, int bn, const void* A, int KP, int M,
                         int Mpad, const void* X, int x_pad, int x_C, int Npix, void* Y,
                         int y_pad, const float* bias, const float* posb, const void* aux,
                         int aux_pad, void* mask, hipStream_t stream);
hipError_t dg_conv_nt(int epi, int kw, int bm, int bn, const void* A, int KP, int M, int Mpad,
                      const void* X, int x_pad, int x_C, int Npix, void* Y, int y_pad,
                      const float* bias, const float* posb, const void* aux, int aux_pad,
                      hipStream_t stream);
void dg_conv_wgrad_set_ablate(int mode);
// the 5x5 weight gradient's kernel: 4 = conv_wgrad_pipe_kernel with four 32-pixel stages,
// 0 = conv_wgrad_kernel (two 64-pixel stages; bit-identical slabs)
void dg_conv_wgrad5_set_ns(int ns);
int dg_conv_wgrad_wgs_per_cu();
// k-tile width / workgroups per CU of the kernel dg_conv_wgrad will use for this K: the
// three-slice kernel wherever K is a multiple of 384
int dg_conv_wgrad_ktile(int KP);
int dg_conv_wgrad_wgs_per_cu_for(int KP);
hipError_t dg_conv_wgrad(int kw, const void* dZ, int dz_pad, int M, int Mpad, const void* X,
                         int x_pad, int x_C, int B, int KP, int splits, float* slab,
                         hipStream_t stream);
// Weight gradients of nl layers of identical geometry in ONE launch (three-slice tiles):
// table = nl rows of {dZ frame, X frame, slab} pointers; each layer gets `splits` pixel
// splits.  Fewer splits per layer than a one-layer launch at the same machine fill, so
// proportionally fewer fp32 partial slabs to write and reduce.
hipError_t dg_conv_wgrad_multi(int kw, const long long* table, int nl, int dz_pad, int M,
                               int Mpad, int x_pad, int x_C, int B, int KP, int splits,
                               hipStream_t stream);
// Slab reduce + bias-gradient pass 2 of one layer; out16 / gposb16 / gbias16 (optional, each
// on its own): bf16 twins of the weight / position-bias / bias gradients.  Refused unless:
// slab (16-byte aligned) and out are given; splits >= 1; 1 <= M <= Mpad; KP > 0 and a multiple
// of 4; taps >= 1; 1 <= cin <= cinp; taps * cinp <= KP (else part of out would never be
// written); M * (KP / 4) fits an int with room for the grid stride; and, when bpart
// (optional) is given, bchunks >= 1 and both gposb and gbias.
hipError_t dg_wgrad_reduce(const float* slab, float* out, int splits, int M, int Mpad, int KP,
                           int taps, int cin, int cinp, const float* bpart, int bchunks,
                           float* gposb, float* gbias, void* out16, void* gposb16,
                           void* gbias16, long long* sf, hipStream_t stream);
// Slab reduce + bias-gradient pass 2 of nl layers (any shapes) in one launch: table = nl
// rows of `cols` int64 {slab, out (weight grad), bpart, gposb, gbias, splits, M, Mpad, KP,
// taps, cin, cinp, bchunks[, out16, gposb16, gbias16]} (cols 13, or 16 with bf16 twins, each
// optional on its own).  1 <= nl <= 16; every row must satisfy dg_wgrad_reduce's rules (the
// int64 columns are checked before they are narrowed) and bpart is required.
hipError_t dg_wgrad_reduce_multi(const long long* table, int nl, int cols, hipStream_t stream);

// ---------------------------------------------------------------- conv_board.hip
// diagnostics: 1 skip MFMA, 2 skip LDS fragment reads, 4 skip DMA
void dg_conv_board_set_ablate(int mode);
// pbias (EPI_FWD, optional): bf16 [361][M] bias + pos_bias table (replaces bias / posb);
// mask (optional): ReLU bitmask [B][361][M/8] — EPI_FWD writes it, EPI_DGRAD gates with it
// instead of reading the aux activation frame.  dg_conv_board = dg_conv_board_ex with neither.
hipError_t dg_conv_board_ex(int epi, int kw, int bm, const void* A, int KP, int M, int Mpad,
                            const void* X, int x_pad, int x_C, int B, void* Y, int y_pad,
                            const float* bias, const float* posb, const void* pbias,
                            const void* aux, int aux_pad, void* mask, hipStream_t stream);
hipError_t dg_conv_board(int epi, int kw, int bm, const void* A, int KP, int M, int Mpad,
                         const void* X, int x_pad, int x_C, int B, void* Y, int y_pad,
                         const float* bias, const float* posb, const void* aux, int aux_pad,
                         hipStream_t stream);

// ---------------------------------------------------------------- conv_stack2.hip
// timing-ablation mode of the forward (tools/kbench_stack.py; 0 = production)
void dg_conv_stack2_set_mode(int on);
// the staggered two-group schedule (overrides DG_STACK2_STAG): 0 off, 1 both stacks, 2 the
// backward-data stack only; co-half-0 MFMA priority 0..2, co-half-1 start delay (s_sleep 127
// rounds)
void dg_conv_stack2_set_sched(int stag, int prio, int delay);
// table: nl rows of {A (fragment-ordered weights), pbias_frag, Y, mask} (int64 pointers)
//   epi 1 (forward): pbias required, mask optional (written)
//   epi 2 (dgrad)  : mask required (read; ReLU bits of the layer below), pbias unused
// l1 (EPI_FWD only): row 0 is the network's first layer (5x5 over the [B][23][23][40] input
// frame X0; its A = the [128][1024] weights in fragment order, k linear)
hipError_t dg_conv_stack2(int epi, const long long* table, int nl, const void* X0, int l1, int B,
                          hipStream_t stream);
// Forward stack + the 3x3 / 128-channel policy head fused after its last layer.
hipError_t dg_conv_stack2_fwd_head(const long long* table, int nl, const void* X0, int l1, int B,
                                   const float* w, const float* bias, const float* posb,
                                   const int* labels, float* loss, int* pred, void* dZ,
                                   float* gw_part, float* dzb, int head_relu, float grad_scale,
                                   hipStream_t stream);
// The same with the feature expansion fused into the first layer's prologue (l1 only): the
// packed batch's planes / player / rank in, the expanded frame X0 written out.
hipError_t dg_conv_stack2_fwd_head_x(const long long* table, int nl, void* X0, int B,
                                     const void* planes, const void* player, const void* rank,
                                     const float* w, const float* bias, const float* posb,
                                     const int* labels, float* loss, int* pred, void* dZ,
                                     float* gw_part, float* dzb, int head_relu, float grad_scale,
                                     hipStream_t stream);

// ---------------------------------------------------------------- conv_layer2.hip
// One hidden 3x3 C -> C layer on conv_stack2's K loop.  epi 1: forward (fragment weights,
// pbias required, mask written if given); 2: backward-data (mask of the layer below
// required).  C = 256 (128 works too: 2 chunks, one workgroup per board).
hipError_t dg_conv_layer2(int epi, const void* A, const void* pbias, const void* X, void* Y,
                          void* mask, int C, int B, hipStream_t stream);
// nl layers in one launch (one workgroup per board, the layers chained through the board's
// own L2-resident output): table = nl rows of {A, pbias, X, Y, mask} (int64); row l + 1's X
// must be row l's Y (checked).  C = 256 | 128 as above.
hipError_t dg_conv_layer2_multi(int epi, const long long* table, int nl, int C, int B,
                                hipStream_t stream);
// the forward run + the fused policy head (3x3 / 256-channel head on the run's last output)
hipError_t dg_conv_layer2_multi_head(const long long* table, int nl, int B, const float* w,
                                     const float* bias, const float* posb, const int* labels,
                                     float* loss, int* pred, void* dZ, float* gw_part,
                                     float* dzb, int head_relu, float grad_scale,
                                     hipStream_t stream);

// ---------------------------------------------------------------- conv_stack_f8.hip
// timing-ablation mode (0 = production)
void dg_conv_stack_f8_set_mode(int m);
// the staggered schedule of C = 128 (overrides DG_STACK_F8_STAG): 0 off, 1 both stacks, 2
// backward-data only; co-half-1 start delay (s_sleep 127 rounds)
void dg_conv_stack_f8_set_sched(int stag, int delay);
// diagnostics: s_memtime phase stamps of boards 0..7 into dbg ([8][8 waves][24 layers][8]
// uint64; null = off; C = 128 production variants)
void dg_conv_stack_f8_set_debug(unsigned long long* dbg);
// The fp8 (MX MFMA) layer stack, C = 128 | 256; X0 is quantized with *s_x0.
// table: nl rows of {A8 (fragment-ordered e4m3 weights), pbias_frag, Y, mask, s_in, s_w,
// s_out, amax_out} (int64); epi 1 forward (e4m3), 2 backward-data (e5m2).
// y8 (optional): nl + 1 int64 {X8_0, Y8 of each layer} fp8 copy-outs (448-row frames); every
// non-last entry present, the last layer's 0.  With y8, Y of the non-last forward layers may
// be null (all or none): the bf16 copy-out is skipped.
// sr_step (backward-data, optional): the int64 device step counter seeding stochastic
// rounding of the e5m2 gradients (null: round to nearest even).
hipError_t dg_conv_stack_f8(int C, int epi, const long long* table, int nl, const void* X0,
                            const float* s_x0, unsigned* amax_x0, int B, const long long* y8,
                            const long long* sr_step, hipStream_t stream);
// The forward stack + the fused 3x3 policy head.  C = 128: the head on the last layer's LDS
// image; 256: on its bf16 frame, read back.
hipError_t dg_conv_stack_f8_fwd_head(int C, const long long* table, int nl, const void* X0,
                                     const float* s_x0, unsigned* amax_x0, int B, const float* w,
                                     const float* bias, const float* posb, const int* labels,
                                     float* loss, int* pred, void* dZ, float* gw_part,
                                     float* dzb, int head_relu, float grad_scale,
                                     const long long* y8, hipStream_t stream);

// ---------------------------------------------------------------- conv_wgrad_win.hip
void dg_conv_wgrad_win_set_ablate(int mode);
// Splits per (layer, chunk pair) that fill num_cus CUs in one round.  At least 8 K-steps per
// split (the prologue loads a full window).
int dg_conv_wgrad_win_splits(int nl, int M, int Cx, int B, int num_cus);
// Sliding-window 3x3 weight gradients (frame-linear K, 9 taps per staged X window):
// table = nl rows of {dZ frame (pad 1, M channels), X frame (pad 1, Cx channels), slab}.
hipError_t dg_conv_wgrad_win(const long long* table, int nl, int M, int Mpad, int Cx, int B,
                             int KP, int splits, long long* sf, hipStream_t stream);

// ---------------------------------------------------------------- conv_wgrad_win8.hip
// timing ablation (tools/kbench_win8.py; 0 = production): 1 no MFMA, 2 no LDS reads, 4 no
// LDS-DMA, 8 no slab store, 16 no barrier (sums of these)
void dg_conv_wgrad_win8_set_ablate(int mode);
// splits per (layer, chunk pair) of dg_conv_wgrad_win8 on num_cus CUs
int dg_conv_wgrad_win8_splits(int nl, int M, int Cx, int B, int num_cus);
// MX-fp8 sliding-window weight gradients: table = nl rows of {dZ8 frame (pad 1, M channels,
// e5m2), X8 frame (pad 1, Cx channels, e4m3), slab, s_dz, s_x} (int64; 448-row fp8 frames).
// B % 4 == 0.
hipError_t dg_conv_wgrad_win8(const long long* table, int nl, int M, int Mpad, int Cx, int B,
                              int KP, int splits, long long* sf, hipStream_t stream);

// ---------------------------------------------------------------- conv_l1.hip
// dg_conv_l1 is usable for: 3x3 / 5x5, pad (k-1)/2 input frame with x_C <= 64 channels
// (multiple of 8), output channels padded to 128, K padded to 64 with zero weights.
int dg_conv_l1_ok(int kw, int x_pad, int x_C, int Mpad, int KP);
// Board-resident first-layer forward: bias + position bias (fp32 bias / posb, or the bf16
// pbias table when given) + ReLU; mask optional.
hipError_t dg_conv_l1(int kw, const void* A, int KP, int M, int Mpad, const void* X, int x_pad,
                      int x_C, int B, void* Y, int y_pad, const float* bias, const float* posb,
                      void* mask, const void* pbias, hipStream_t stream);
// conv_l1_frag: 5x5 over the [B][23][23][40] input frame -> [B][21][21][M] (pad 1), M a
// multiple of 128, one board per workgroup; A = weight_refresh's fragment-ordered first-layer
// operand, pbias = its stack-order bias table; mask optional.  planes / player / rank
// (optional, all or none): the feature expansion fused in (X written instead of read).
int dg_conv_l1_frag_ok(int kw, int x_pad, int x_C, int M, int y_pad);
hipError_t dg_conv_l1_frag(const void* A, const void* pbias, void* X, int B, int M, void* Y,
                           void* mask, const void* planes, const void* player, const void* rank,
                           hipStream_t stream);

// ---------------------------------------------------------------- conv_fp8.hip
hipError_t dg_conv_board_fp8(int kw, int bm, const void* A8, int KP, int M, int Mpad,
                             const void* X8, int x_pad, int x_C, int B, void* Y, void* Y8,
                             int y_pad, const float* bias, const float* posb, const float* s_x,
                             const float* s_w, const float* s_y, unsigned* amax_y, void* mask,
                             hipStream_t stream);
hipError_t dg_fp8_update_scales(int n, float* scales, unsigned* amax_w, int nparts_w,
                                unsigned* amax_y, float w_margin, float g_headroom, int* sat,
                                float* gscales, unsigned* gamax, float* ghist, hipStream_t s);
hipError_t dg_weight_fp8(const float* w, void* wf8, int cout, int cin, int taps, int cinp, int kp,
                         const float* s_w, hipStream_t s);
hipError_t dg_frame_to_fp8(const void* src, void* dst, size_t n, const float* scale,
                           unsigned* amax, hipStream_t s);

// ---------------------------------------------------------------- head.hip, head_mfma.hip
// gw16 / gbias16 / gposb16 (optional): bf16 twins of the reduced gradients
hipError_t dg_head_reduce(const float* dzb, const float* gw_part, int B, int n, float* gw,
                          float* gbias, float* gposb, void* gw16, void* gbias16, void* gposb16,
                          long long* sf, hipStream_t stream);
// The policy head (forward, loss, argmax and the block's backward).  `unused` is ignored: the
// slot remains because it is part of the recorded head(...) call.
hipError_t dg_head(int kw, const void* X, int x_pad, int C, int B, const float* w,
                   const float* bias, const float* posb, const int* labels, float* loss,
                   int* pred, float* logp_out, void* dZ, int dz_pad, float* gw_part,
                   float* unused, float* dzb, int head_relu, float grad_scale,
                   hipStream_t stream);
// 3x3 head over a 128- or 256-channel pad-1 frame (the 12-layer configs); called by dg_head,
// not bound to Python.
hipError_t dg_head_mfma(int C, const void* X, int B, const float* w, const float* bias,
                        const float* posb, const int* labels, float* loss, int* pred,
                        float* logp_out, void* dZ, float* gw_part, float* dzb, int head_relu,
                        float grad_scale, hipStream_t stream);

// ---------------------------------------------------------------- elementwise.hip
// out2 / CP2: a second output frame (optional; null, 0 from Python)
hipError_t dg_expand_features(const uint8_t* planes, const uint8_t* player, const uint8_t* rank,
                              void* out, int B, int pad, int CP, void* out2, int CP2,
                              hipStream_t s);
// part must hold nchunks*(361 + 19)*C floats, nchunks = dg_bias_chunks(B) = ceil(B / 16)
hipError_t dg_bias_grad_partial(const void* dZ, int B, int C, int pad, float* part,
                                hipStream_t s);
// Pass 1 for nl same-shape layers in one launch: table = nl rows of {dZ frame, part, s8}
// (s8: 0 = bf16 frame, else the e5m2 copy's scale pointer; pad must be 1 then);
// chunks of dg_bias_chunks_multi(B) boards.
hipError_t dg_bias_grad_partial_multi(const long long* table, int nl, int B, int C, int pad,
                                      long long* sf, hipStream_t s);
int dg_bias_chunks(int B);
int dg_bias_chunks_multi(int B);
// g16 (optional): read the bf16 twin gradient instead of g (data-parallel bf16 wire)
hipError_t dg_sgd(float* p, const float* g, size_t n, const double* lr, float gscale,
                  const float* gate, const void* g16, hipStream_t s);
hipError_t dg_rmsprop(float* p, const float* g, float* ms, size_t n, const double* lr,
                      float decay, float gscale, const float* gate, const void* g16,
                      hipStream_t s);
// loss (optional, rank-local) and grads (optional, flat, all-reduced; or its bf16 twin
// grads16) -> gate in {0, 1}
hipError_t dg_finite_gate(const float* loss, int n, const float* grads, size_t ng, float* gate,
                          int* bad_count, const void* grads16, hipStream_t s);
// gate = finite(loss) && finite(grads | grads16) in one launch (gate_all_kernel); ticket: one
// zeroed word the launch leaves zeroed
hipError_t dg_finite_gate1(const float* loss, int n, const float* grads, const void* grads16,
                           size_t ng, float* gate, int* bad_count, unsigned* ticket,
                           hipStream_t s);
hipError_t dg_lr_decay(double* lr, double decay, long long* step, hipStream_t s);
// Operand refresh of n layers.  table: n rows of 20 int64 words
//   {w, wf, wd, cout, cin, taps, cinp, kpf, kpd, pbias_frag, wf8, s_w, amax_w, bias, posb,
//    pbias, wf_frag, wd_frag, wf8_frag, wd8_frag}  (pbias_frag / *_frag: stack-order tables,
//    or 0; a null copy output is not written)
// lr (optional): fused per-step decay lr *= (1 - decay), step += 1 (see the kernel).
hipError_t dg_weight_refresh(const long long* table, int n, double* lr, double decay,
                             long long* step, hipStream_t s);
// The fused gradient pass 2 + optimizer + refresh (grad_update_kernel).  table: n rows of
// dg_grad_update_cols() = 29 int64 = the 20 weight_refresh columns, then {slab, bpart,
// splits, Mpad, KP, bchunks, w_off, b_off, pos_off} (slab / bpart 0: the layer's gradient is
// read from G / G16).  plain_off / plain_n: a flat range updated from G only (the head).
// tickets: dg_grad_update_tickets() zeroed uint32 (left zeroed).  write_grads: with slabs,
// also store the reduced gradient in G.  Tile blocks per row = dg_weight_refresh's block
// count (the fp8 |w| max slots), plus GU_NB bias blocks per 64-channel block of the widest
// layer.
int dg_grad_update_cols();
int dg_grad_update_tickets();
hipError_t dg_grad_update(const long long* table, int n, long long plain_off, long long plain_n,
                          float* P, float* G, const void* G16, float* MS, float rms_decay,
                          float gscale, const float* gate, double* lr, double decay,
                          long long* step, unsigned* tickets, int* bad_steps, int write_grads,
                          int final, const long long* gflag, hipStream_t s);
// nbytes of a bucket (multiple of 16), world = the ring size it stands in for, gbps = link
// rate (GB/s; 0 = unpaced), blocks = channel workgroups
hipError_t dg_comm_proxy(void* buf, long long nbytes, int world, double gbps, int blocks,
                         hipStream_t s);

// ---------------------------------------------------------------- policy.hip
// Boards i S + s of a packed batch <- source board i moved by symmetry s.  The four
// destinations are the views of a packed batch buffer (data/batch.py) of capacity B >= n S
// boards.
hipError_t dg_symmetry_planes(const uint8_t* src_planes, const uint8_t* src_player,
                              const uint8_t* src_rank, const int* src_labels, int n, int S,
                              uint8_t* planes, uint8_t* player, uint8_t* rank, int* labels,
                              int B, hipStream_t s);
// Symmetry-averaged, legality-masked policy with top-k and label rank.
// logp [n S][361]; stones: plane 0 of the UNtransformed positions, board stride
// stones_stride bytes; extra_illegal [n][361] (nonzero = illegal) and labels [n] optional.
hipError_t dg_policy_ensemble(const float* logp, const uint8_t* stones, int stones_stride,
                              const uint8_t* extra_illegal, const int* labels, int n, int S,
                              int K, int mask, float* prob, int* topk_idx, float* topk_p,
                              int* label_rank, hipStream_t s);

// ---------------------------------------------------------------- augment.hip (module _dgaug)
// Every board i < B of a packed batch (planes [B][9][361], labels [B]) moved IN PLACE by the
// board symmetry s_i: sym[i] & 7 when sym (optional, uint8 [B]) is given, else
// dg_augment_symmetry(seed, seq, board0 + i).  A label in 0..360 becomes T_s(label), any other
// value stays; a board with s = 0 is not written.  sym_out (optional, uint8 [B]): the ids used.
hipError_t dg_augment_batch(uint8_t* planes, int* labels, int B, const uint8_t* sym,
                            unsigned long long seed, unsigned long long seq,
                            unsigned long long board0, uint8_t* sym_out, hipStream_t stream);
// The hash behind it, on the host (data/symmetry.py augment_symmetries is the definition).
int dg_augment_symmetry(unsigned long long seed, unsigned long long seq,
                        unsigned long long board);

// ---------------------------------------------------------------- play.hip (module _dgplay)
// One move per position from policy_ensemble's prob [n][361] (masked and normalised), tempered
// by `temperature` and cut to the top_p nucleus; the draw of position i is
// dg_select_uniform(seed, game[i], ply[i]).  move [n]: the point, -1 for a row without a legal
// point or with a non-finite or negative entry; p_move [n] (optional): the tempered,
// renormalised probability of the chosen point; kept [n] (optional): the size of the nucleus (0
// / -1 for those two kinds of row).  deep_go_amd/play/select.py is the definition.  Refused
// before any GPU work: n < 0; a null prob, game, ply or move; temperature < 0 or not finite;
// top_p outside (0, 1].
hipError_t dg_policy_select(const float* prob, const int* game, const int* ply, int n,
                            unsigned long long seed, float temperature, float top_p, int* move,
                            float* p_move, int* kept, hipStream_t stream);
// The draw behind it, on the host: u in [0, 1) on the 2^-24 grid (play/select.py
// select_uniform is the definition).
float dg_select_uniform(unsigned long long seed, int game, int ply);

// ---------------------------------------- optim.hip (modules _dgopt, _dgadam and _dglamb)
// SGD with momentum over the flat vector, one launch: gi = g * gscale; gw = gi + wd * p inside
// a decay range, else gi; v = mu * v + gw; p -= lr * (nesterov ? gw + mu * v : v).  ranges: a
// HOST array of n_ranges <= 20 rows {begin, end} (elements; sorted, disjoint, non-empty, begin
// a multiple of 64, end <= n and below 2^32 - 1), passed to the kernel by value.  gate / g16
// as dg_sgd; p, v, g 16-byte aligned (g16: 8).  lr is read, not written: the decay stays with
// dg_weight_refresh.
hipError_t dg_momentum(float* p, const float* g, float* v, size_t n, const double* lr, float mu,
                       int nesterov, float wd, const long long* ranges, int n_ranges,
                       float gscale, const float* gate, const void* g16, hipStream_t s);

// AdamW over the flat vector (module _dgadam): gi = g * gscale; m = beta1 m + (1 - beta1) gi;
// v = beta2 v + (1 - beta2) gi^2; p *= 1 - lr wd inside a decay range; p -= lr c1 m /
// (sqrt(v) c2 + eps).  rec: the optimizer's 16-byte device record {int64 t; float c1; float c2}
// (8-byte aligned), t the count of APPLIED steps.  Two launches on s: dg_adamw_tick (one wave:
// behind an open gate t += 1, c1 = 1 / (1 - beta1^t), c2 = 1 / sqrt(1 - beta2^t), in double;
// nothing behind a closed one), then the update, which only reads c1 and c2.  gate 0 leaves p,
// m, v and rec untouched.  ranges, gate, g16, lr and the alignment of p, m, v, g as
// dg_momentum; beta1, beta2 in [0, 1), eps > 0.
hipError_t dg_adamw_tick(void* rec, float beta1, float beta2, const float* gate, hipStream_t s);
hipError_t dg_adamw(float* p, const float* g, float* m, float* v, size_t n, const double* lr,
                    void* rec, float beta1, float beta2, float eps, float wd,
                    const long long* ranges, int n_ranges, float gscale, const float* gate,
                    const void* g16, hipStream_t s);

// LAMB over the flat vector (module _dglamb): Adam's m, v as dg_adamw; u = (c1 m) / (sqrt(v) c2
// + eps), + wd p inside a range; per range k of the table SP = sum p^2, SU = sum u^2 (each
// rounded to fp32), wn = sqrt(SP), un = sqrt(SU) (fp32), phi = fp32(double(wn) / double(un))
// if both are finite and > 0, else 1; p -= (lr phi) u, phi = 1 outside every range.  Four
// launches on s: dg_adamw_tick on rec (as dg_adamw), lamb_moments (m, v, u and per 1024-element
// chunk and range meeting it one fp32 pair of partial sums), lamb_ratio (one workgroup per
// range: the pairs summed in double, {wn, un, phi} to row k of tab), lamb_apply.  No atomics,
// one fixed order: the same input gives the same bits on any grid.  u: n floats of scratch,
// 16-byte aligned; part: part_n >= dg_lamb_partials(n, ranges, n_ranges) floats, 8-byte
// aligned; tab: 20 x 3 floats.  dg_lamb_partials returns -1 for an invalid table or one with
// more than 4 ranges meeting one chunk, which dg_lamb refuses too.  gate 0 leaves p, m, v, u,
// rec, part and tab untouched.  Everything else as dg_adamw.
long long dg_lamb_partials(size_t n, const long long* ranges, int n_ranges);
hipError_t dg_lamb(float* p, const float* g, float* m, float* v, float* u, size_t n,
                   const double* lr, void* rec, float* part, long long part_n, float* tab,
                   float beta1, float beta2, float eps, float wd, const long long* ranges,
                   int n_ranges, float gscale, const float* gate, const void* g16,
                   hipStream_t s);

// ---------------------------------------------------------------- clip.hip (module _dgclip)
// Global-norm gradient clipping over the flat gradient: norm = |gscale| sqrt(sum g^2); r =
// max_norm / (norm + 1e-6); scale = r < 1 ? r : 1; g *= scale (the optimizer behind it still
// applies gscale).  Two launches on s: up to dg_clip_partials() workgroups each write one fp32
// partial of the sum of squares to part (part_n >= dg_clip_partials() floats), then every
// workgroup sums the partials in double in one fixed order and scales its share.  No atomics:
// the same input gives the same bits.  rec: the 16-byte device record {float norm; float scale;
// int64 clipped} (8-byte aligned), clipped += 1 when scale < 1.  Exactly one of g (fp32,
// 16-byte aligned: scaled in place, untouched when scale == 1; out must be null) and g16 (the
// bf16 wire twin, 8-byte aligned: only read; out[i] = scale * float(g16[i]) is always written,
// out fp32 and 16-byte aligned).  gate 0 leaves g, out, part and rec untouched.  max_norm > 0
// and finite, gscale finite; n == 0 launches nothing.
int dg_clip_partials();
hipError_t dg_grad_clip(float* g, const void* g16, float* out, size_t n, float* part,
                        int part_n, void* rec, float max_norm, float gscale, const float* gate,
                        hipStream_t s);
// the first launch alone: part[b] for b below min(ceil(floor(n / 4) / 256), dg_clip_partials()),
// at least one; sum them for sum g^2
hipError_t dg_grad_norm(const float* g, const void* g16, size_t n, float* part, int part_n,
                        const float* gate, hipStream_t s);

// ------------------------------------------------------------------ ema.hip (module _dgema)
// An exponential moving average e of the flat parameter vector p, once per APPLIED step:
// t += 1; d = min(decay, (1 + t) / (10 + t)) in double; omd = float(1 - d); e[i] = fmaf(omd,
// p[i] - e[i], e[i]).  rec: the average's 16-byte device record {int64 t; float omd; float pad}
// (8-byte aligned), t the count of applied steps.  Two launches on s: dg_ema_tick (one wave:
// behind an open gate t += 1 and omd; nothing behind a closed one), then the average, which
// only reads omd and p.  gate 0 leaves e and rec untouched.  p, e 16-byte aligned and not null,
// decay in [0, 1); n == 0 launches nothing.
hipError_t dg_ema_tick(void* rec, double decay, const float* gate, hipStream_t s);
hipError_t dg_ema(const float* p, float* e, size_t n, void* rec, double decay, const float* gate,
                  hipStream_t s);

// --------------------------------------------------------------- sched.hip (module _dgsched)
// The learning-rate schedule: one launch (lr_sched_tick: one wave, one lane, NO gate: a skipped
// step counts) on rec, the 16-byte device record {double base; int64 s} (8-byte aligned), and
// lr, the rate the optimizer kernels read.  advance 1: base *= (1 - rate_decay); s += 1; *lr =
// base * f(s).  advance 0: *lr = base * f(s) only.  f(s) = w(s) d(s) of
// deep_go_amd/train/optim.py lr_factor; kind 0 constant | 1 linear | 2 cosine | 3 step; W >= 0,
// T >= 0 (linear, cosine: T > W), m in [0, 1], E >= 0 (step: E > 0), g in (0, 1], rate_decay
// finite; anything else is refused before any GPU work.
hipError_t dg_lr_sched(void* rec, double* lr, int kind, long long W, long long T, double m,
                       long long E, double g, double rate_decay, int advance, hipStream_t s);

}  // extern "C"
