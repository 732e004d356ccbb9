/*
 * pgx_actor_host.cpp -- the Actor's argument checks and the host model of its arithmetic.
 *
 * pgx_actor_forward_host restates, in plain C++ on host arrays, what pgx_actor.hip's forward kernel
 * computes up to the squash: the feature order, every Linear as one k-ordered std::fmaf chain that
 * starts at the bias and runs over K rounded up to 16 (include/pgx.h, "Arithmetic contract"), the
 * ReLU, clip_mean and the log_std clamp.  On gfx950 the f32-input MFMA is such a chain bit for
 * bit, so the kernel is tested against this on the device and this against an independent
 * restatement on a CPU.  Never touches a device; the Actor does not step through it.
 * pgx_ac_forward_host (below) is the same for pgx_actor_critic.hip: both trunks and heads of the
 * ActorCritic over the same `linear`.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/pgx.h"

int pgx_set_error(int code, const char* msg);  /* pgx_api.cpp: sets pgx_last_error() */

/* pgx_actor_create's checks (no device call); `what` names the entry point */
int pgx_actor_check_config(const pgx_actor_config* c, const char* what, bool with_envs) {
    char msg[160];
    auto bad = [&](const char* field) {
        snprintf(msg, sizeof(msg), "%s: %s", what, field);
        return pgx_set_error(PGX_E_INVALID, msg);
    };
    if (!c) return bad("null config");
    if (with_envs && c->n_envs <= 0) return bad("n_envs must be > 0");
    if (c->obs_dim <= 0 || c->obs_dim > 4096) return bad("obs_dim must be in 1..4096");
    if (c->action_dim < 1 || c->action_dim > PGX_ACTOR_MAX_ACTION) return bad("action_dim must be in 1..7");
    if (c->n_layers < 1 || c->n_layers > PGX_ACTOR_MAX_LAYERS) return bad("n_layers must be in 1..3");
    for (int l = 0; l < c->n_layers; l++)
        if (c->hidden[l] < 1 || c->hidden[l] > PGX_ACTOR_MAX_WIDTH) return bad("hidden widths must be in 1..512");
    if (c->kind != PGX_ACTOR_GAUSSIAN && c->kind != PGX_ACTOR_DETERMINISTIC) return bad("unknown kind");
    if (!(c->clip_mean >= 0.0) || std::isinf(c->clip_mean)) return bad("clip_mean must be finite and >= 0");
    if (!(c->noise_sigma >= 0.0) || std::isinf(c->noise_sigma)) return bad("noise_sigma must be finite and >= 0");
    if (!std::isfinite(c->noise_mu)) return bad("noise_mu must be finite");
    return PGX_OK;
}

namespace {

/* y[o] = chain(bias[o]; x[k] * W[o][k], k ascending over K rounded up to 16), optionally ReLU */
void linear(const float* W, const float* b, const float* x, int K, int out, bool relu, float* y) {
    const int K16 = (K + 15) & ~15;
    for (int o = 0; o < out; o++) {
        float acc = b[o];
        for (int k = 0; k < K; k++) acc = std::fmaf(x[k], W[(size_t)o * K + k], acc);
        for (int k = K; k < K16; k++) acc = std::fmaf(0.0f, 0.0f, acc);
        y[o] = relu ? (acc > 0.0f ? acc : 0.0f) : acc;
    }
}

}  // namespace

extern "C" int pgx_actor_forward_host(const pgx_actor_config* cfg, const pgx_actor_weights* w, const float* obs,
                                      const float* achieved_goal, const float* desired_goal, int32_t n, float* mean_out,
                                      float* log_std_out) {
    const char* what = "pgx_actor_forward_host";
    const int rc = pgx_actor_check_config(cfg, what, false);
    if (rc != PGX_OK) return rc;
    if (!w || !obs || !achieved_goal || !desired_goal || !mean_out || n < 0)
        return pgx_set_error(PGX_E_INVALID, "pgx_actor_forward_host: null pointer or n < 0");
    const int nl = cfg->n_layers, A = cfg->action_dim, od = cfg->obs_dim;
    const int heads = cfg->kind == PGX_ACTOR_GAUSSIAN ? 2 : 1;
    for (int l = 0; l < nl + heads; l++)
        if (!w->weight[l] || !w->bias[l])
            return pgx_set_error(PGX_E_INVALID, "pgx_actor_forward_host: null weight or bias pointer");
    const float clip = (float)cfg->clip_mean;
    std::vector<float> x(od + 6), y(PGX_ACTOR_MAX_WIDTH), z(PGX_ACTOR_MAX_WIDTH);
    for (int32_t e = 0; e < n; e++) {
        for (int k = 0; k < 3; k++) x[k] = achieved_goal[(size_t)e * 3 + k];
        for (int k = 0; k < 3; k++) x[3 + k] = desired_goal[(size_t)e * 3 + k];
        for (int k = 0; k < od; k++) x[6 + k] = obs[(size_t)e * od + k];
        const float* in = x.data();
        int K = od + 6;
        float* out = y.data();
        for (int l = 0; l < nl; l++) {
            linear(w->weight[l], w->bias[l], in, K, cfg->hidden[l], true, out);
            in = out;
            K = cfg->hidden[l];
            out = out == y.data() ? z.data() : y.data();
        }
        float head[PGX_ACTOR_MAX_ACTION];
        linear(w->weight[nl], w->bias[nl], in, K, A, false, head);
        for (int d = 0; d < A; d++) {
            float m = head[d];
            if (clip > 0.0f) m = m < -clip ? -clip : (m > clip ? clip : m);
            mean_out[(size_t)e * A + d] = m;
        }
        if (heads == 2 && log_std_out) {
            linear(w->weight[nl + 1], w->bias[nl + 1], in, K, A, false, head);
            for (int d = 0; d < A; d++) {
                const float v = head[d];
                log_std_out[(size_t)e * A + d] =
                    v < PGX_ACTOR_LOG_STD_MIN ? PGX_ACTOR_LOG_STD_MIN : (v > PGX_ACTOR_LOG_STD_MAX ? PGX_ACTOR_LOG_STD_MAX : v);
            }
        }
    }
    return PGX_OK;
}

/* ---------------------------------------------------------------- ActorCritic (include/pgx.h) */

/* pgx_ac_create's checks (no device call); `what` names the entry point */
int pgx_ac_check_config(const pgx_ac_config* c, const char* what, bool with_envs) {
    char msg[160];
    auto bad = [&](const char* field) {
        snprintf(msg, sizeof(msg), "%s: %s", what, field);
        return pgx_set_error(PGX_E_INVALID, msg);
    };
    if (!c) return bad("null config");
    if (with_envs && c->n_envs <= 0) return bad("n_envs must be > 0");
    if (c->obs_dim <= 0 || c->obs_dim > 4096) return bad("obs_dim must be in 1..4096");
    if (c->action_dim < 1 || c->action_dim > PGX_ACTOR_MAX_ACTION) return bad("action_dim must be in 1..7");
    if (c->n_pi_layers < 1 || c->n_pi_layers > PGX_ACTOR_MAX_LAYERS) return bad("n_pi_layers must be in 1..3");
    if (c->n_vf_layers < 1 || c->n_vf_layers > PGX_ACTOR_MAX_LAYERS) return bad("n_vf_layers must be in 1..3");
    for (int l = 0; l < c->n_pi_layers; l++)
        if (c->pi_hidden[l] < 1 || c->pi_hidden[l] > PGX_ACTOR_MAX_WIDTH) return bad("pi_hidden widths must be in 1..512");
    for (int l = 0; l < c->n_vf_layers; l++)
        if (c->vf_hidden[l] < 1 || c->vf_hidden[l] > PGX_ACTOR_MAX_WIDTH) return bad("vf_hidden widths must be in 1..512");
    return PGX_OK;
}

extern "C" int pgx_ac_forward_host(const pgx_ac_config* cfg, const pgx_ac_weights* w, const float* obs,
                                   const float* achieved_goal, const float* desired_goal, int32_t n, float* mean_out,
                                   float* value_out) {
    const char* what = "pgx_ac_forward_host";
    const int rc = pgx_ac_check_config(cfg, what, false);
    if (rc != PGX_OK) return rc;
    if (!w || !obs || !achieved_goal || !desired_goal || n < 0)
        return pgx_set_error(PGX_E_INVALID, "pgx_ac_forward_host: null pointer or n < 0");
    const int A = cfg->action_dim, od = cfg->obs_dim;
    for (int l = 0; l < cfg->n_pi_layers; l++)
        if (!w->pi_weight[l] || !w->pi_bias[l])
            return pgx_set_error(PGX_E_INVALID, "pgx_ac_forward_host: null pi_weight or pi_bias pointer");
    for (int l = 0; l < cfg->n_vf_layers; l++)
        if (!w->vf_weight[l] || !w->vf_bias[l])
            return pgx_set_error(PGX_E_INVALID, "pgx_ac_forward_host: null vf_weight or vf_bias pointer");
    if (!w->action_net_weight || !w->action_net_bias || !w->value_net_weight || !w->value_net_bias)
        return pgx_set_error(PGX_E_INVALID, "pgx_ac_forward_host: null action_net or value_net pointer");
    std::vector<float> x(od + 6), y(PGX_ACTOR_MAX_WIDTH), z(PGX_ACTOR_MAX_WIDTH);
    /* one trunk and its head over x: out_dim outputs into head */
    auto trunk = [&](int nl, const int32_t* hidden, const float* const* W, const float* const* b, const float* hw,
                     const float* hb, int out_dim, float* head) {
        const float* in = x.data();
        int K = od + 6;
        float* out = y.data();
        for (int l = 0; l < nl; l++) {
            linear(W[l], b[l], in, K, hidden[l], true, out);
            in = out;
            K = hidden[l];
            out = out == y.data() ? z.data() : y.data();
        }
        linear(hw, hb, in, K, out_dim, false, head);
    };
    for (int32_t e = 0; e < n; e++) {
        for (int k = 0; k < 3; k++) x[k] = achieved_goal[(size_t)e * 3 + k];
        for (int k = 0; k < 3; k++) x[3 + k] = desired_goal[(size_t)e * 3 + k];
        for (int k = 0; k < od; k++) x[6 + k] = obs[(size_t)e * od + k];
        float head[PGX_ACTOR_MAX_ACTION];
        if (mean_out) {
            trunk(cfg->n_pi_layers, cfg->pi_hidden, w->pi_weight, w->pi_bias, w->action_net_weight, w->action_net_bias, A,
                  head);
            for (int d = 0; d < A; d++) mean_out[(size_t)e * A + d] = head[d];
        }
        if (value_out) {
            trunk(cfg->n_vf_layers, cfg->vf_hidden, w->vf_weight, w->vf_bias, w->value_net_weight, w->value_net_bias, 1,
                  head);
            value_out[e] = head[0];
        }
    }
    return PGX_OK;
}

/* ---------------------------------------------------------------- SdeActor (include/pgx.h) */

/* pgx_sde_actor_create's checks (no device call); `what` names the entry point */
int pgx_sde_actor_check_config(const pgx_sde_actor_config* c, const char* what, bool with_envs) {
    char msg[160];
    auto bad = [&](const char* field) {
        snprintf(msg, sizeof(msg), "%s: %s", what, field);
        return pgx_set_error(PGX_E_INVALID, msg);
    };
    if (!c) return bad("null config");
    if (with_envs && c->n_envs <= 0) return bad("n_envs must be > 0");
    if (c->obs_dim <= 0 || c->obs_dim > 4096) return bad("obs_dim must be in 1..4096");
    if (c->action_dim < 1 || c->action_dim > PGX_ACTOR_MAX_ACTION) return bad("action_dim must be in 1..7");
    if (c->n_layers < 1 || c->n_layers > PGX_ACTOR_MAX_LAYERS) return bad("n_layers must be in 1..3");
    for (int l = 0; l < c->n_layers; l++)
        if (c->hidden[l] < 1 || c->hidden[l] > PGX_ACTOR_MAX_WIDTH) return bad("hidden widths must be in 1..512");
    if (!(c->clip_mean >= 0.0) || std::isinf(c->clip_mean)) return bad("clip_mean must be finite and >= 0");
    return PGX_OK;
}

extern "C" int pgx_sde_actor_forward_host(const pgx_sde_actor_config* cfg, const pgx_sde_actor_weights* w,
                                          const float* obs, const float* achieved_goal, const float* desired_goal,
                                          const float* matrices, int32_t n, float* mean_out, float* latent_out,
                                          float* noise_out) {
    const char* what = "pgx_sde_actor_forward_host";
    const int rc = pgx_sde_actor_check_config(cfg, what, false);
    if (rc != PGX_OK) return rc;
    if (!w || !obs || !achieved_goal || !desired_goal || n < 0)
        return pgx_set_error(PGX_E_INVALID, "pgx_sde_actor_forward_host: null pointer or n < 0");
    if (noise_out && !matrices)
        return pgx_set_error(PGX_E_INVALID, "pgx_sde_actor_forward_host: null matrices with noise_out");
    const int nl = cfg->n_layers, A = cfg->action_dim, od = cfg->obs_dim, H = cfg->hidden[nl - 1];
    for (int l = 0; l <= nl; l++)
        if (!w->weight[l] || !w->bias[l])
            return pgx_set_error(PGX_E_INVALID, "pgx_sde_actor_forward_host: null weight or bias pointer");
    const float clip = (float)cfg->clip_mean;
    std::vector<float> x(od + 6), y(PGX_ACTOR_MAX_WIDTH), z(PGX_ACTOR_MAX_WIDTH);
    for (int32_t e = 0; e < n; e++) {
        for (int k = 0; k < 3; k++) x[k] = achieved_goal[(size_t)e * 3 + k];
        for (int k = 0; k < 3; k++) x[3 + k] = desired_goal[(size_t)e * 3 + k];
        for (int k = 0; k < od; k++) x[6 + k] = obs[(size_t)e * od + k];
        const float* in = x.data();
        int K = od + 6;
        float* out = y.data();
        for (int l = 0; l < nl; l++) {
            linear(w->weight[l], w->bias[l], in, K, cfg->hidden[l], true, out);
            in = out;
            K = cfg->hidden[l];
            out = out == y.data() ? z.data() : y.data();
        }
        const float* latent = in;
        if (latent_out)
            for (int h = 0; h < H; h++) latent_out[(size_t)e * H + h] = latent[h];
        if (mean_out) {
            float head[PGX_ACTOR_MAX_ACTION];
            linear(w->weight[nl], w->bias[nl], latent, H, A, false, head);
            for (int d = 0; d < A; d++) {
                float m = head[d];
                if (clip > 0.0f) m = m < -clip ? -clip : (m > clip ? clip : m);
                mean_out[(size_t)e * A + d] = m;
            }
        }
        if (noise_out) {
            const float* E = matrices + (size_t)e * H * A;
            for (int d = 0; d < A; d++) {
                float acc = 0.0f;   /* one chain, exactly H terms */
                for (int h = 0; h < H; h++) acc = std::fmaf(latent[h], E[(size_t)h * A + d], acc);
                noise_out[(size_t)e * A + d] = acc;
            }
        }
    }
    return PGX_OK;
}
