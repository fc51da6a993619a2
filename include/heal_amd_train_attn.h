/* heal_amd_train_attn.h -- entry points of the TRAINING side of CoBEVT's agent-window attention.
 *
 * The inference ABI (include/heal_amd.h, HEAL_AMD_ABI_VERSION) stays as it is; the kernels declared here are shipped in the same
 * library (every build exports them) and serve the opt-in kernel-backed backward of the swap fusion
 * (heal_amd.ops.AgentWindowAttention, Attention.grad_kernel / CoBEVT's `grad_kernel` argument).
 * Same conventions as include/heal_amd.h: device pointers, fp32, a hipStream_t as void*, non-zero return + heal_last_error() on
 * failure, no host synchronisation (safe under graph capture), workspaces supplied by the caller.
 */
#ifndef HEAL_AMD_TRAIN_ATTN_H
#define HEAL_AMD_TRAIN_ATTN_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* heal_agent_window_attention_backward: the gradient of heal_agent_window_attention (include/heal_amd.h; same shapes, layouts,
 *   token order (l w1 w2), modes and masking).  With G = (H / 4)(W / 4) groups of T = 16 n_agents tokens and, per group and head,
 *   P = softmax(scale Q K^T + bias[h]) over the keys of the agents < n_valid:
 *     dV = P^T dO,   dP = dO V^T,   dS = P o (dP - rowsum(dO o O)),   dQ = scale dS K,   dK = scale dS^T Q,
 *     dbias[h] = sum over the groups of dS.
 *   rowsum(dO o O) is formed as sum_j P_j dP_j from the recomputed tiles (the same number; as the mean of the dP values it is
 *   subtracted from it cancels against them, which measurably lowers the error of the gradients that reach the LayerNorm before
 *   the attention), so the forward's output is not an argument.
 *   qkv [n_agents,H,W,3,heads,32], bias [heads,T,T] or null, grad_out [n_agents,H,W,heads*32],
 *   grad_qkv like qkv, grad_bias [heads,T,T] (required exactly when bias is given); all 16-B aligned.
 *   Every token belongs to one group, so grad_qkv is written by plain stores: all of it, need not be initialised.  Keys of agents
 *   >= n_valid are neither loaded nor multiplied: their dK / dV rows and their columns of grad_bias are written as exact zeros and
 *   whatever their K / V hold (NaN included) reaches no output.  Their QUERIES are not masked: dQ of padded agents is computed.
 *   One block (one wave per agent, Q / K / V / dO of a group in LDS) per (part, head) walks the groups of its part: a query-owned
 *   phase recomputes the scores as the forward does, keeps (max, 1 / sum, sum_j P_j dP_j) per query in LDS and produces dQ and dS; a
 *   key-owned phase rebuilds P^T / dS^T from those and produces dV and dK.  No [G,heads,T,T] tensor exists in memory.
 *   grad_bias is deterministic: the G groups are cut into `parts` contiguous ranges (G % parts leading ranges hold one group more
 *   than the rest), a block sums dS over its range in registers and, with parts > 1, writes its partial [part][heads][T][T] to ws;
 *   a second launch adds the partials in part order.  No floating-point atomics: repeated launches are bit-equal.
 *   parts: 1..G, or 0 for heal_agent_window_attention_backward_parts(...) = min(G, max(1, 1024 / heads)) (a pure function of the
 *   shape; never an empty part).  ws: heal_agent_window_attention_backward_workspace(...) bytes = parts * heads * T * T * 4 for
 *   parts > 1 (parts = 0: the policy's value), 0 for one part or an unsupported shape; not needed (may be null) when bias is null.
 *   _supported: 1 <= n_agents <= HEAL_AGENT_WINDOW_MAX_AGENTS, window 4, dim_head 32, H and W positive multiples of 4.            */
int heal_agent_window_attention_backward_supported(int n_agents, int window, int dim_head, int H, int W);
int heal_agent_window_attention_backward_parts(int n_agents, int H, int W, int heads);
size_t heal_agent_window_attention_backward_workspace(int n_agents, int H, int W, int heads, int parts);
int heal_agent_window_attention_backward(const float* qkv, const float* bias, const float* grad_out, int n_agents, int n_valid,
                                         int H, int W, int heads, int dim_head, int window, int mode, float scale,
                                         int parts, float* grad_qkv, float* grad_bias, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
