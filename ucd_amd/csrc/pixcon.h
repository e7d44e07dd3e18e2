// Internal constants shared by the contrastive kernels.
#pragma once
#include "common.h"

namespace ucd {
// Row granularity of the contrast matrix: the anchor segment and the teacher segment are each padded
// to a multiple of this many rows (padding rows carry label 255 and zero features).
constexpr int kPixTile = 128;
constexpr int kPadLabel = 255;

// Host-side plan of one ucd_pixcon_loss call: which kernels serve it and with what launch parameters.  ucd_pixcon_loss_plan
// reports it and every launch takes its numbers from it (pixcon_make_plan, pixcon_loss.hip; no device call).
struct PixconPlan {
  int path;              // enum ucd_pixcon_path
  int class_chunk;       // classes per staged piece of the probability product; 0: all classes in one piece
  int kp;                // class count as the probability product pads it (even: fp32, multiple of 16: fp16); 0 without use_prob
  int nt_i;              // anchor blocks of 128 rows
  int nsplit1, nsplit2;  // grid.y of the two sweeps; 0 for the planned form (persistent workgroups draw units)
  size_t lds1, lds2;     // dynamic LDS bytes of sweep 1 / sweep 2
  size_t workspace;      // bytes the path lays out in the workspace
};
// validates (BHW, K, precision, temperature) and fills *p; returns 0 or the code ucd_pixcon_loss returns for these arguments
int pixcon_make_plan(const char* fn, int BHW, int K, int precision, int use_prob, float temperature, PixconPlan* p);

// fp16-operand loss path, fixed split (pixcon_loss_f16.hip).  A launch takes the call's plan: sizes, LDS bytes and
// p->kp = KP16 come from it, and the caller has checked the workspace against p->workspace.
void pixcon16_plan(int BHW, int KP16, PixconPlan* p);
int pixcon16_launch(const _Float16* ch16, const uint8_t* row_label, const _Float16* p16, const ucd_pixcon_meta* meta, int BHW,
                    float temperature, int shift_pos, int use_prob, float* loss_out, float* grad_a, int ldg, float* row_stats,
                    void* workspace, const PixconPlan& p, hipStream_t s);
// planned, software-pipelined form of the same path (pixcon_loss_f16p.hip); eligible for T >= 0.06, at most 32 teacher
// classes and fewer than 1024 anchor blocks
bool pixcon16p_eligible(int BHW, float temperature, int use_prob, int K);
void pixcon16p_plan(int BHW, int KP16, int use_prob, PixconPlan* p);
size_t pixcon16p_workspace_bytes(int BHW);
int pixcon16p_launch(const _Float16* ch16, const uint8_t* row_label, const _Float16* p16, const ucd_pixcon_meta* meta, int BHW,
                     float temperature, int shift_pos, int use_prob, float* loss_out, float* grad_a, int ldg, float* row_stats,
                     void* workspace, const PixconPlan& p, hipStream_t s);
// loss_out[0] = sum(row_loss[0:A]) / n_valid, loss_out[1] = n_valid (pixcon_loss.hip)
void pixcon_launch_reduce(const float* row_loss, const ucd_pixcon_meta* meta, float* loss_out, hipStream_t s);
}  // namespace ucd
