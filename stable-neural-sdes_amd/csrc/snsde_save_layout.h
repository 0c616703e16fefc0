// The save format of a training solve: the slots per pass of act_save / delta_save and what each slot holds.  The forward kernels that
// write the planes, the adjoints, the weight- and coefficient-gradient passes that read them and snsde_save_layout, from which the
// caller sizes them, all take it from here.  DESIGN.md section 2 has the map as a table.
//   NHID = num_hidden_layers - 1;  NN = layers of the diffusion net on [tau, y] (0, 1, 2);  method = SNSDE_EULER / _MILSTEIN / _SRK (SRK:
//   three passes per step, pass 3n + 2 also holds the step's fourth, "tail", net evaluation);  smooth = the activation is not relu
#pragma once
#include "snsde.h"
namespace snsde_save {
#define SNSDE_SAVE_FN __host__ __device__ constexpr int
// ---- slots per pass.  act_save: layer outputs [+ pre-activations: smooth];  delta_save: the same count [+ Milstein's factors of the
// second-order parameter terms through a net].  snsde_save_layout reports delta_slots + pre_slots: the caller's delta buffer has
// act_save's slot count, so under a smooth activation it ends in room no kernel touches (the kernels stride by delta_slots)
SNSDE_SAVE_FN act_slots(int NHID, int NN, int method) { return NHID + 2 + NN + (method == SNSDE_SRK ? NN : 0); }
SNSDE_SAVE_FN pre_slots(int NHID, int NN, int method, bool smooth) { return smooth ? NHID + 1 + (NN == 2 ? (method == SNSDE_SRK ? 2 : 1) : 0) : 0; }
SNSDE_SAVE_FN nsave(int NHID, int NN, int method, bool smooth) { return act_slots(NHID, NN, method) + pre_slots(NHID, NN, method, smooth); }
SNSDE_SAVE_FN stage_planes(int NN, int method) { return method == SNSDE_SRK && NN > 0 ? 3 : 1; }
SNSDE_SAVE_FN milstein_slots(int NN, int method) { return method == SNSDE_MILSTEIN && NN > 0 ? (NN == 2 ? 3 : 1) : 0; }
SNSDE_SAVE_FN delta_slots(int NHID, int NN, int method) { return act_slots(NHID, NN, method) + milstein_slots(NN, method); }
// ---- act_save slots
SNSDE_SAVE_FN act_layer(int k) { return k; }                                  // output of the first layer (k = 0) / hidden layer k (1 .. NHID)
SNSDE_SAVE_FN act_z(int NHID) { return NHID + 1; }                            // pre-tanh drift; relu: sign bits in its low mantissa bits (below)
SNSDE_SAVE_FN act_net(int NHID, int l) { return NHID + 2 + l; }               // diffusion net, layer l (NN == 2: hidden, output)
SNSDE_SAVE_FN act_net_out(int NHID, int NN) { return act_net(NHID, NN - 1); }
SNSDE_SAVE_FN act_tail(int NHID, int NN, int l) { return act_net(NHID, NN + l); }      // SRK: the tail evaluation's
SNSDE_SAVE_FN act_tail_out(int NHID, int NN) { return act_tail(NHID, NN, NN - 1); }
// smooth: pre-activation k; k = 0 .. NHID the drift's layers, pre_net the net's hidden layer, pre_tail the tail's
SNSDE_SAVE_FN act_pre(int NHID, int NN, int method, int k) { return act_slots(NHID, NN, method) + k; }
SNSDE_SAVE_FN pre_net(int NHID) { return NHID + 1; }        SNSDE_SAVE_FN pre_tail(int NHID) { return NHID + 2; }
// ---- delta_save slots: dL/d (a layer's output before its activation), in the adjoint's order - output side first
SNSDE_SAVE_FN delta_out(void) { return 0; }                                   // the pre-tanh drift
SNSDE_SAVE_FN delta_hidden(int NHID, int l) { return NHID - l; }              // hidden layer l = 0 .. NHID - 1 (its input is act_layer(l))
SNSDE_SAVE_FN delta_first(int NHID) { return NHID + 1; }                      // the drift's first layer
SNSDE_SAVE_FN delta_net(int NHID, int j) { return NHID + 2 + j; }             // diffusion net, j layers before its output layer
SNSDE_SAVE_FN delta_net_in(int NHID, int NN) { return delta_net(NHID, NN - 1); }      // ... its layer on [tau, y]
SNSDE_SAVE_FN delta_tail(int NHID, int NN, int j) { return delta_net(NHID, NN + j); }
SNSDE_SAVE_FN delta_tail_in(int NHID, int NN) { return delta_tail(NHID, NN, NN - 1); }
// Milstein's factors: eps2, eps1, hdot (NN == 2) | eps (NN == 1, in eps2's slot); eps_y is the one that multiplies the net's y input
SNSDE_SAVE_FN delta_eps2(int NHID, int NN) { return act_slots(NHID, NN, SNSDE_MILSTEIN); }
SNSDE_SAVE_FN delta_eps1(int NHID, int NN) { return delta_eps2(NHID, NN) + 1; }
SNSDE_SAVE_FN delta_hdot(int NHID, int NN) { return delta_eps2(NHID, NN) + 2; }
SNSDE_SAVE_FN delta_eps_y(int NHID, int NN) { return NN == 2 ? delta_eps1(NHID, NN) : delta_eps2(NHID, NN); }
// ---- relu sign bits packed into the saved z (snsde_pack_signs): bit k = [act_layer(k) > 0]; the diffusion-net tiles and the wave
// pairs add, for a two-layer net under Milstein / SRK, [net hidden > 0] and (SRK, pass 3n + 2) the tail's
SNSDE_SAVE_FN drift_sign_bits(int NHID) { return NHID + 1; }
SNSDE_SAVE_FN net_sign_bit(int NHID) { return NHID + 1; }   SNSDE_SAVE_FN tail_sign_bit(int NHID) { return NHID + 2; }
SNSDE_SAVE_FN sign_bits(int NHID, int NN, int method) { return drift_sign_bits(NHID) + (NN == 2 ? (method == SNSDE_SRK ? 2 : (method == SNSDE_MILSTEIN ? 1 : 0)) : 0); }
#undef SNSDE_SAVE_FN
}  // namespace snsde_save
