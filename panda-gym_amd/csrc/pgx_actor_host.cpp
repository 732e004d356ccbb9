/*
 * pgx_actor_host.cpp -- the policy units' argument checks and the host models of their arithmetic.
 *
 * pgx_actor_forward_host restates, in plain C++ on host arrays, what pgx_actor.hip's forward kernel
 * computes up to the squash: the feature order, every Linear as one k-ordered std::fmaf chain that
 * starts at the bias and runs over K rounded up to 16 (include/pgx.h, "Arithmetic contract"), the
 * ReLU, clip_mean and the log_std clamp.  On gfx950 the f32-input MFMA is such a chain bit for
 * bit, so the kernel is tested against this on the device and this against an independent
 * restatement on a CPU.  Never touches a device; the Actor does not step through it.
 * pgx_ac_forward_host and pgx_sde_actor_forward_host (below) are the same for pgx_actor_critic.hip and
 * pgx_sde_actor.hip, over the same `stage_row`, `hidden_layers` and `linear`; the check_config share
 * `check_dims`, `check_common`, `check_count` and `check_widths`.  `stage_row` is every model's stager: it reads each
 * field through a row stride, (obs_dim, 3, 3) for the dense per-env models, with the action columns for the quantile
 * critics.  The three batch launch checks share `check_rows_ptrs` and `check_rows_shape`, each launch's own pointers
 * checked between the two, so the message that wins for any set of bad fields is the one that always did.  pgx_qc_forward_host and pgx_qc_target_host (last) are
 * the quantile critics' (pgx_quantile_critic.hip): the same Linears, then the pooled sort by the order
 * rule's key, the truncation and the unfused Bellman backup; the launch checks they share with the device
 * entry points are pgx_qc_check_launch.  pgx_actor_log_prob_host and pgx_sde_actor_log_prob_host are the
 * action log-probability entries' contracts (the Actor's and the SdeActor's batch launches): the forward's
 * planes, the padded noise and variance chains of the gSDE distribution, and the unfused epilogues through
 * the host's libm; their launch checks, pgx_actor_lp_check_launch and pgx_sde_actor_lp_check_launch, are the
 * device entries' too.  pgx_qc_critic_grad_host and pgx_qc_adam_step_host (last) restate the critic update:
 * the quantile Huber loss, the Linears' backward and Adam in the header's orders, behind
 * pgx_qc_check_grad_launch and pgx_qc_check_adam, which the device entries call as well.
 */
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/pgx.h"

int pgx_set_error(int code, const char* msg);  /* pgx_api.cpp: sets pgx_last_error() */

namespace {

int bad(const char* what, const char* field, const char* rest = "") {
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: %s%s", what, field, rest);
    return pgx_set_error(PGX_E_INVALID, msg);
}

/* what the four configs share, ... */
int check_dims(const char* what, int obs_dim, int action_dim) {
    if (obs_dim <= 0 || obs_dim > 4096) return bad(what, "obs_dim must be in 1..4096");
    if (action_dim < 1 || action_dim > PGX_ACTOR_MAX_ACTION) return bad(what, "action_dim must be in 1..7");
    return PGX_OK;
}

/* ... and the three that hold per-env state */
template <class Config>
int check_common(const Config* c, const char* what, bool with_envs) {
    if (!c) return bad(what, "null config");
    if (with_envs && c->n_envs <= 0) return bad(what, "n_envs must be > 0");
    return check_dims(what, c->obs_dim, c->action_dim);
}

/* a stack's layer count, then its widths; `name` is the config field's */
int check_count(const char* what, const char* name, int n) {
    return n < 1 || n > PGX_ACTOR_MAX_LAYERS ? bad(what, name, " must be in 1..3") : PGX_OK;
}

int check_widths(const char* what, const char* name, int n, const int32_t* widths) {
    for (int l = 0; l < n; l++)
        if (widths[l] < 1 || widths[l] > PGX_ACTOR_MAX_WIDTH) return bad(what, name, " widths must be in 1..512");
    return PGX_OK;
}

int check_clip_mean(const char* what, double clip_mean) {
    return !(clip_mean >= 0.0) || std::isinf(clip_mean) ? bad(what, "clip_mean must be finite and >= 0") : PGX_OK;
}

int up16(int n) { return (n + 15) / 16 * 16; }

float clip_to(float m, float clip) { return clip > 0.0f ? (m < -clip ? -clip : (m > clip ? clip : m)) : m; }

float clamp_log_std(float v) {
    return v < PGX_ACTOR_LOG_STD_MIN ? PGX_ACTOR_LOG_STD_MIN : (v > PGX_ACTOR_LOG_STD_MAX ? PGX_ACTOR_LOG_STD_MAX : v);
}

/* What the three batch launches' checks share, each launch's own pointers checked in between: io and the
 * pointers every one of them reads ... */
template <class Io>
int check_rows_ptrs(const Io* io, const char* what) {
    if (!io) return bad(what, "null io");
    if (!io->obs) return bad(what, "null obs");
    if (!io->achieved_goal) return bad(what, "null achieved_goal");
    if (!io->desired_goal) return bad(what, "null desired_goal");
    if (!io->action) return bad(what, "null action");
    return PGX_OK;
}

/* ... and B and the observation fields' row strides */
template <class Io>
int check_rows_shape(const Io* io, int32_t B, int obs_dim, const char* what) {
    if (B <= 0) return bad(what, "B must be > 0");
    if (io->obs_stride < obs_dim) return bad(what, "obs_stride is below obs_dim");
    if (io->achieved_goal_stride < 3) return bad(what, "achieved_goal_stride is below 3");
    if (io->desired_goal_stride < 3) return bad(what, "desired_goal_stride is below 3");
    return PGX_OK;
}

}  // namespace

/* pgx_actor_create's checks (no device call); `what` names the entry point */
int pgx_actor_check_config(const pgx_actor_config* c, const char* what, bool with_envs) {
    int rc = check_common(c, what, with_envs);
    if (rc == PGX_OK) rc = check_count(what, "n_layers", c->n_layers);
    if (rc == PGX_OK) rc = check_widths(what, "hidden", c->n_layers, c->hidden);
    if (rc != PGX_OK) return rc;
    if (c->kind != PGX_ACTOR_GAUSSIAN && c->kind != PGX_ACTOR_DETERMINISTIC) return bad(what, "unknown kind");
    if ((rc = check_clip_mean(what, c->clip_mean)) != PGX_OK) return rc;
    if (!(c->noise_sigma >= 0.0) || std::isinf(c->noise_sigma)) return bad(what, "noise_sigma must be finite and >= 0");
    if (!std::isfinite(c->noise_mu)) return bad(what, "noise_mu must be finite");
    return PGX_OK;
}

namespace {

/* y[o] = chain(bias[o]; x[k] * W[o][k], k ascending over K rounded up to 16), optionally ReLU */
void linear(const float* W, const float* b, const float* x, int K, int out, bool relu, float* y) {
    const int K16 = up16(K);
    for (int o = 0; o < out; o++) {
        float acc = b[o];
        for (int k = 0; k < K; k++) acc = std::fmaf(x[k], W[(size_t)o * K + k], acc);
        for (int k = K; k < K16; k++) acc = std::fmaf(0.0f, 0.0f, acc);
        y[o] = relu ? (acc > 0.0f ? acc : 0.0f) : acc;
    }
}

/* x [od + 6 + ad] = achieved_goal | desired_goal | observation | action of row b, each field through its row
 * stride (floats): (od, 3, 3) for the dense per-env inputs; ad = 0: no action columns */
void stage_row(float* x, const float* obs, const float* achieved_goal, const float* desired_goal, int s_obs, int s_ag,
               int s_dg, size_t b, int od, const float* action = nullptr, int s_act = 0, int ad = 0) {
    for (int k = 0; k < 3; k++) x[k] = achieved_goal[b * s_ag + k];
    for (int k = 0; k < 3; k++) x[3 + k] = desired_goal[b * s_dg + k];
    for (int k = 0; k < od; k++) x[6 + k] = obs[b * s_obs + k];
    for (int k = 0; k < ad; k++) x[6 + od + k] = action[b * s_act + k];
}

/* the same from a batch launch's io (the action, which the two actors' io only writes, is the caller's to name) */
template <class Io>
void stage_row(float* x, const Io* io, size_t b, int od, const float* action = nullptr, int s_act = 0, int ad = 0) {
    stage_row(x, io->obs, io->achieved_goal, io->desired_goal, io->obs_stride, io->achieved_goal_stride,
              io->desired_goal_stride, b, od, action, s_act, ad);
}

/* the nl hidden Linears with their ReLU over x [in_dim], y and z taking turns as output; returns the
 * last one's output, [hidden[nl - 1]] */
const float* hidden_layers(int nl, const int32_t* hidden, const float* const* W, const float* const* b, const float* x,
                           int in_dim, float* y, float* z) {
    const float* in = x;
    int K = in_dim;
    float* out = y;
    for (int l = 0; l < nl; l++) {
        linear(W[l], b[l], in, K, hidden[l], true, out);
        in = out;
        K = hidden[l];
        out = out == y ? z : y;
    }
    return in;
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
    const int K = cfg->hidden[nl - 1];
    for (int32_t e = 0; e < n; e++) {
        stage_row(x.data(), obs, achieved_goal, desired_goal, od, 3, 3, (size_t)e, od);
        const float* in = hidden_layers(nl, cfg->hidden, w->weight, w->bias, x.data(), od + 6, y.data(), z.data());
        float head[PGX_ACTOR_MAX_ACTION];
        linear(w->weight[nl], w->bias[nl], in, K, A, false, head);
        for (int d = 0; d < A; d++) mean_out[(size_t)e * A + d] = clip_to(head[d], clip);
        if (heads == 2 && log_std_out) {
            linear(w->weight[nl + 1], w->bias[nl + 1], in, K, A, false, head);
            for (int d = 0; d < A; d++) log_std_out[(size_t)e * A + d] = clamp_log_std(head[d]);
        }
    }
    return PGX_OK;
}

namespace {

/* what the two action_log_prob launches share: io's pointers and strides, B */
template <class Io>
int check_lp_io(const Io* io, int32_t B, int obs_dim, const char* what) {
    const int rc = check_rows_ptrs(io, what);
    if (rc != PGX_OK) return rc;
    if (!io->log_prob) return bad(what, "null log_prob");
    return check_rows_shape(io, B, obs_dim, what);
}

/* the epilogues of include/pgx.h, every operation rounded on its own but the one fmaf */
#pragma clang fp contract(off)
void lp_terms(float mean, float ls, float eps, float* g, float* act, float* lp, float* c) {
    const float std = std::exp(ls);
    *g = std::fmaf(std, eps, mean);
    const float t = std::tanh(*g);
    const float z = *g - mean;
    *lp = ((-(z * z)) / (2.0f * (std * std)) - ls) - 0.9189385f;
    *c = std::log((1.0f - t * t) + 1e-6f);
    *act = t;
}

void sde_lp_terms(float mean, float noise, float var, float* act, float* gp, float* lp, float* c) {
    const float scale = std::sqrt(var + 1e-6f);
    const float a = std::tanh(mean + noise);
    const float lim = 1.0f - 1.1920929e-7f;
    const float x = a < -lim ? -lim : (a > lim ? lim : a);
    const float g = 0.5f * (std::log1p(x) - std::log1p(-x));
    const float z = g - mean;
    *lp = ((-(z * z)) / (2.0f * (scale * scale)) - std::log(scale)) - 0.9189385f;
    const float t = std::tanh(g);
    *c = std::log((1.0f - t * t) + 1e-6f);
    *act = a;
    *gp = g;
}

/* (lp_0 + lp_1 + ...) - (c_0 + c_1 + ...), each sum from its first term in ascending d */
float sum_log_prob(const float* lp, const float* c, int A) {
    float s_lp = lp[0], s_c = c[0];
    for (int d = 1; d < A; d++) {
        s_lp = s_lp + lp[d];
        s_c = s_c + c[d];
    }
    return s_lp - s_c;
}
#pragma clang fp contract(on)

}  // namespace

/* the checks of one pgx_actor_action_log_prob launch, device and host alike */
int pgx_actor_lp_check_launch(const pgx_actor_config* c, const pgx_actor_lp_io* io, int32_t B, const char* what) {
    if (c->kind != PGX_ACTOR_GAUSSIAN) return bad(what, "kind must be PGX_ACTOR_GAUSSIAN: a DETERMINISTIC actor has no log-probability");
    return check_lp_io(io, B, c->obs_dim, what);
}

extern "C" int pgx_actor_log_prob_host(const pgx_actor_config* cfg, const pgx_actor_weights* w, const pgx_actor_lp_io* io,
                                       int32_t n) {
    const char* what = "pgx_actor_log_prob_host";
    int rc = pgx_actor_check_config(cfg, what, false);
    if (rc == PGX_OK) rc = pgx_actor_lp_check_launch(cfg, io, n, what);
    if (rc != PGX_OK) return rc;
    if (!io->eps) return bad(what, "null eps");
    if (!w) return bad(what, "null weights");
    const int nl = cfg->n_layers, A = cfg->action_dim, od = cfg->obs_dim, K = cfg->hidden[nl - 1];
    for (int l = 0; l < nl + 2; l++)
        if (!w->weight[l] || !w->bias[l]) return bad(what, "null weight or bias pointer");
    const float clip = (float)cfg->clip_mean;
    std::vector<float> x(od + 6), y(PGX_ACTOR_MAX_WIDTH), z(PGX_ACTOR_MAX_WIDTH);
    for (int32_t b = 0; b < n; b++) {
        stage_row(x.data(), io, (size_t)b, od);
        const float* in = hidden_layers(nl, cfg->hidden, w->weight, w->bias, x.data(), od + 6, y.data(), z.data());
        float mu[PGX_ACTOR_MAX_ACTION], ls[PGX_ACTOR_MAX_ACTION], lp[PGX_ACTOR_MAX_ACTION], c[PGX_ACTOR_MAX_ACTION];
        linear(w->weight[nl], w->bias[nl], in, K, A, false, mu);
        linear(w->weight[nl + 1], w->bias[nl + 1], in, K, A, false, ls);
        for (int d = 0; d < A; d++) {
            const size_t o = (size_t)b * A + d;
            const float mean = clip_to(mu[d], clip);
            const float log_std = clamp_log_std(ls[d]);
            float g, act;
            lp_terms(mean, log_std, io->eps[o], &g, &act, &lp[d], &c[d]);
            io->action[o] = act;
            if (io->mean_out) io->mean_out[o] = mean;
            if (io->log_std_out) io->log_std_out[o] = log_std;
            if (io->eps_out) io->eps_out[o] = io->eps[o];
            if (io->gaussian_action_out) io->gaussian_action_out[o] = g;
        }
        io->log_prob[b] = sum_log_prob(lp, c, A);
    }
    return PGX_OK;
}

/* ---------------------------------------------------------------- ActorCritic (include/pgx.h) */

/* pgx_ac_create's checks (no device call); `what` names the entry point */
int pgx_ac_check_config(const pgx_ac_config* c, const char* what, bool with_envs) {
    int rc = check_common(c, what, with_envs);
    if (rc == PGX_OK) rc = check_count(what, "n_pi_layers", c->n_pi_layers);
    if (rc == PGX_OK) rc = check_count(what, "n_vf_layers", c->n_vf_layers);
    if (rc == PGX_OK) rc = check_widths(what, "pi_hidden", c->n_pi_layers, c->pi_hidden);
    if (rc == PGX_OK) rc = check_widths(what, "vf_hidden", c->n_vf_layers, c->vf_hidden);
    return rc;
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
        const float* in = hidden_layers(nl, hidden, W, b, x.data(), od + 6, y.data(), z.data());
        linear(hw, hb, in, hidden[nl - 1], out_dim, false, head);
    };
    for (int32_t e = 0; e < n; e++) {
        stage_row(x.data(), obs, achieved_goal, desired_goal, od, 3, 3, (size_t)e, od);
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
    int rc = check_common(c, what, with_envs);
    if (rc == PGX_OK) rc = check_count(what, "n_layers", c->n_layers);
    if (rc == PGX_OK) rc = check_widths(what, "hidden", c->n_layers, c->hidden);
    if (rc == PGX_OK) rc = check_clip_mean(what, c->clip_mean);
    return rc;
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
        stage_row(x.data(), obs, achieved_goal, desired_goal, od, 3, 3, (size_t)e, od);
        const float* latent = hidden_layers(nl, cfg->hidden, w->weight, w->bias, x.data(), od + 6, y.data(), z.data());
        if (latent_out)
            for (int h = 0; h < H; h++) latent_out[(size_t)e * H + h] = latent[h];
        if (mean_out) {
            float head[PGX_ACTOR_MAX_ACTION];
            linear(w->weight[nl], w->bias[nl], latent, H, A, false, head);
            for (int d = 0; d < A; d++) mean_out[(size_t)e * A + d] = clip_to(head[d], clip);
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

/* the checks of one pgx_sde_actor_action_log_prob launch, device and host alike */
int pgx_sde_actor_lp_check_launch(const pgx_sde_actor_config* c, const pgx_sde_actor_lp_io* io, int32_t B,
                                  const char* what) {
    return check_lp_io(io, B, c->obs_dim, what);
}

extern "C" int pgx_sde_actor_log_prob_host(const pgx_sde_actor_config* cfg, const pgx_sde_actor_weights* w,
                                           const float* std_ha, const float* exploration_mat,
                                           const pgx_sde_actor_lp_io* io, int32_t n) {
    const char* what = "pgx_sde_actor_log_prob_host";
    int rc = pgx_sde_actor_check_config(cfg, what, false);
    if (rc == PGX_OK) rc = pgx_sde_actor_lp_check_launch(cfg, io, n, what);
    if (rc != PGX_OK) return rc;
    if (!exploration_mat) return bad(what, "null exploration_mat");
    if (!w) return bad(what, "null weights");
    const int nl = cfg->n_layers, A = cfg->action_dim, od = cfg->obs_dim, H = cfg->hidden[nl - 1];
    for (int l = 0; l <= nl; l++)
        if (!w->weight[l] || !w->bias[l]) return bad(what, "null weight or bias pointer");
    if (!std_ha && !w->log_std) return bad(what, "null std and log_std");
    const int K16 = up16(H);
    std::vector<float> std2((size_t)H * A);
    for (size_t j = 0; j < std2.size(); j++) {
        const float s = std_ha ? std_ha[j] : std::exp(w->log_std[j]);
        std2[j] = s * s;
    }
    const float clip = (float)cfg->clip_mean;
    std::vector<float> x(od + 6), y(PGX_ACTOR_MAX_WIDTH), z(PGX_ACTOR_MAX_WIDTH);
    for (int32_t b = 0; b < n; b++) {
        stage_row(x.data(), io, (size_t)b, od);
        const float* latent = hidden_layers(nl, cfg->hidden, w->weight, w->bias, x.data(), od + 6, y.data(), z.data());
        if (io->latent_out)
            for (int h = 0; h < H; h++) io->latent_out[(size_t)b * H + h] = latent[h];
        float mu[PGX_ACTOR_MAX_ACTION], lp[PGX_ACTOR_MAX_ACTION], c[PGX_ACTOR_MAX_ACTION];
        linear(w->weight[nl], w->bias[nl], latent, H, A, false, mu);
        for (int d = 0; d < A; d++) {
            float noise = 0.0f, var = 0.0f;   /* the Linear chain with bias +0, padded to K16 */
            for (int h = 0; h < H; h++) {
                noise = std::fmaf(latent[h], exploration_mat[(size_t)h * A + d], noise);
                const float sq = latent[h] * latent[h];
                var = std::fmaf(sq, std2[(size_t)h * A + d], var);
            }
            for (int h = H; h < K16; h++) {
                noise = std::fmaf(0.0f, 0.0f, noise);
                var = std::fmaf(0.0f, 0.0f, var);
            }
            const size_t o = (size_t)b * A + d;
            const float mean = clip_to(mu[d], clip);
            float act, g;
            sde_lp_terms(mean, noise, var, &act, &g, &lp[d], &c[d]);
            io->action[o] = act;
            if (io->mean_out) io->mean_out[o] = mean;
            if (io->noise_out) io->noise_out[o] = noise;
            if (io->variance_out) io->variance_out[o] = var;
            if (io->gaussian_action_out) io->gaussian_action_out[o] = g;
        }
        io->log_prob[b] = sum_log_prob(lp, c, A);
    }
    return PGX_OK;
}

/* ---------------------------------------------------------------- QuantileCritic (include/pgx.h) */

/* pgx_qc_create's checks (no device call); `what` names the entry point */
int pgx_qc_check_config(const pgx_qc_config* c, const char* what) {
    if (!c) return bad(what, "null config");
    int rc = check_dims(what, c->obs_dim, c->action_dim);
    if (rc == PGX_OK) rc = check_count(what, "n_layers", c->n_layers);
    if (rc == PGX_OK) rc = check_widths(what, "hidden", c->n_layers, c->hidden);
    if (rc != PGX_OK) return rc;
    if (c->n_critics < 1 || c->n_critics > PGX_QC_MAX_CRITICS) return bad(what, "n_critics must be in 1..5");
    if (c->n_quantiles < 1 || c->n_quantiles > PGX_QC_MAX_QUANTILES) return bad(what, "n_quantiles must be in 1..32");
    if (c->n_critics * c->n_quantiles > PGX_QC_MAX_POOL) return bad(what, "n_critics * n_quantiles must be <= 128");
    if (!std::isfinite(c->gamma)) return bad(what, "gamma must be finite");
    return PGX_OK;
}

/* the checks of one launch, pgx_qc_forward's (target false) or pgx_qc_target's, device and host alike */
int pgx_qc_check_launch(const pgx_qc_config* c, const pgx_qc_io* io, int32_t B, bool target, int32_t n_target,
                        const char* what) {
    int rc = check_rows_ptrs(io, what);
    if (rc != PGX_OK) return rc;
    if (!io->out) return bad(what, "null out");
    if ((rc = check_rows_shape(io, B, c->obs_dim, what)) != PGX_OK) return rc;
    if (io->action_stride < c->action_dim) return bad(what, "action_stride is below action_dim");
    if (!target) return PGX_OK;
    if (!io->reward) return bad(what, "null reward");
    if (!io->done) return bad(what, "null done");
    if (!io->next_log_prob) return bad(what, "null next_log_prob");
    if (!io->ent_coef) return bad(what, "null ent_coef");
    if (n_target < 1 || n_target > c->n_critics * c->n_quantiles) return bad(what, "n_target must be in 1..n_critics * n_quantiles");
    if (io->reward_stride < 1) return bad(what, "reward_stride is below 1");
    if (io->done_stride < 1) return bad(what, "done_stride is below 1");
    return PGX_OK;
}

int pgx_qc_check_weights(const pgx_qc_config* c, const pgx_qc_weights* w, const char* what) {
    if (!w) return bad(what, "null weights");
    for (int i = 0; i < c->n_critics; i++)
        for (int l = 0; l <= c->n_layers; l++)
            if (!w->weight[i][l] || !w->bias[i][l]) return bad(what, "null weight or bias pointer");
    return PGX_OK;
}

namespace {

/* the order rule's key of an f32's bits */
uint32_t qc_key(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

/* row b's T quantiles, [critic][quantile], of the set w */
void qc_row(const pgx_qc_config* cfg, const pgx_qc_weights* w, const pgx_qc_io* io, size_t b, float* x, float* y,
            float* zz, float* out) {
    const int od = cfg->obs_dim, A = cfg->action_dim, nl = cfg->n_layers, nq = cfg->n_quantiles;
    stage_row(x, io, b, od, io->action, io->action_stride, A);
    for (int c = 0; c < cfg->n_critics; c++) {
        const float* in = hidden_layers(nl, cfg->hidden, w->weight[c], w->bias[c], x, od + 6 + A, y, zz);
        linear(w->weight[c][nl], w->bias[c][nl], in, cfg->hidden[nl - 1], nq, false, out + (size_t)c * nq);
    }
}

/* the epilogue of the truncated target: four operations, four roundings */
#pragma clang fp contract(off)
float qc_backup(float z, float ent_coef, float next_log_prob, float reward, float done, float gamma) {
    const float t1 = ent_coef * next_log_prob;
    const float t2 = z - t1;
    const float m = (1.0f - done) * gamma;
    return reward + m * t2;
}
#pragma clang fp contract(on)

}  // namespace

extern "C" int pgx_qc_forward_host(const pgx_qc_config* cfg, const pgx_qc_weights* w, const pgx_qc_io* io, int32_t B) {
    const char* what = "pgx_qc_forward_host";
    int rc = pgx_qc_check_config(cfg, what);
    if (rc == PGX_OK) rc = pgx_qc_check_weights(cfg, w, what);
    if (rc == PGX_OK) rc = pgx_qc_check_launch(cfg, io, B, false, 0, what);
    if (rc != PGX_OK) return rc;
    const int T = cfg->n_critics * cfg->n_quantiles;
    std::vector<float> x(cfg->obs_dim + 6 + cfg->action_dim), y(PGX_ACTOR_MAX_WIDTH), z(PGX_ACTOR_MAX_WIDTH);
    for (int32_t b = 0; b < B; b++) qc_row(cfg, w, io, (size_t)b, x.data(), y.data(), z.data(), io->out + (size_t)b * T);
    return PGX_OK;
}

extern "C" int pgx_qc_target_host(const pgx_qc_config* cfg, const pgx_qc_weights* w, const pgx_qc_io* io, int32_t B,
                                  int32_t n_target) {
    const char* what = "pgx_qc_target_host";
    int rc = pgx_qc_check_config(cfg, what);
    if (rc == PGX_OK) rc = pgx_qc_check_weights(cfg, w, what);
    if (rc == PGX_OK) rc = pgx_qc_check_launch(cfg, io, B, true, n_target, what);
    if (rc != PGX_OK) return rc;
    const int T = cfg->n_critics * cfg->n_quantiles;
    const float ent = *io->ent_coef, gamma = (float)cfg->gamma;
    std::vector<float> x(cfg->obs_dim + 6 + cfg->action_dim), y(PGX_ACTOR_MAX_WIDTH), zz(PGX_ACTOR_MAX_WIDTH);
    float q[PGX_QC_MAX_POOL];
    int order[PGX_QC_MAX_POOL];
    for (int32_t b = 0; b < B; b++) {
        qc_row(cfg, w, io, (size_t)b, x.data(), y.data(), zz.data(), q);
        if (io->quantiles_out)
            for (int i = 0; i < T; i++) io->quantiles_out[(size_t)b * T + i] = q[i];
        for (int i = 0; i < T; i++) order[i] = i;
        /* stable: equal keys keep their flat-index order */
        std::stable_sort(order, order + T, [&q](int i, int j) { return qc_key(q[i]) < qc_key(q[j]); });
        for (int k = 0; k < n_target; k++)
            io->out[(size_t)b * n_target + k] =
                qc_backup(q[order[k]], ent, io->next_log_prob[b], io->reward[(size_t)b * io->reward_stride],
                          io->done[(size_t)b * io->done_stride], gamma);
    }
    return PGX_OK;
}

/* ---------------------------------------------------------------- QuantileCritic, the critic update */

/* floats of one workspace row: x [K16] | per critic A_0 .. A_{nl-1}, dZ_0 .. dZ_nl (widths up to 16) | 16 */
int64_t pgx_qc_grad_row_floats(const pgx_qc_config* c) {
    int64_t per_critic = up16(c->n_quantiles);
    for (int l = 0; l < c->n_layers; l++) per_critic += 2 * up16(c->hidden[l]);
    return up16(c->obs_dim + 6 + c->action_dim) + c->n_critics * per_critic + 16;
}

extern "C" int64_t pgx_qc_grad_workspace_floats(const pgx_qc_config* cfg, int32_t B) {
    const char* what = "pgx_qc_grad_workspace_floats";
    const int rc = pgx_qc_check_config(cfg, what);
    if (rc != PGX_OK) return rc;
    if (B <= 0) return bad(what, "B must be > 0");
    return (int64_t)B * pgx_qc_grad_row_floats(cfg);
}

/* the checks of one pgx_qc_critic_grad launch, device and host alike */
int pgx_qc_check_grad_launch(const pgx_qc_config* c, const pgx_qc_grad_io* io, int32_t B, int32_t n_target,
                             const char* what) {
    int rc = check_rows_ptrs(io, what);
    if (rc != PGX_OK) return rc;
    if (!io->target_quantiles) return bad(what, "null target_quantiles");
    if (!io->workspace) return bad(what, "null workspace");
    if (!io->loss) return bad(what, "null loss");
    if ((rc = check_rows_shape(io, B, c->obs_dim, what)) != PGX_OK) return rc;
    if (io->action_stride < c->action_dim) return bad(what, "action_stride is below action_dim");
    if (n_target < 1 || n_target > c->n_critics * c->n_quantiles) return bad(what, "n_target must be in 1..n_critics * n_quantiles");
    if (io->workspace_floats < (int64_t)B * pgx_qc_grad_row_floats(c))
        return bad(what, "workspace_floats is below pgx_qc_grad_workspace_floats(cfg, B)");
    return PGX_OK;
}

/* pgx_qc_init_training's and the host Adam's constants */
int pgx_qc_check_adam(double beta1, double beta2, double eps, const char* what) {
    if (!(beta1 >= 0.0 && beta1 < 1.0)) return bad(what, "beta1 must be in [0, 1)");
    if (!(beta2 >= 0.0 && beta2 < 1.0)) return bad(what, "beta2 must be in [0, 1)");
    if (!(eps > 0.0) || std::isinf(eps)) return bad(what, "eps must be finite and > 0");
    return PGX_OK;
}

float pgx_qc_inv_count(const pgx_qc_config* c, int32_t B, int32_t n_target) {
    return 1.0f / (float)((int64_t)B * c->n_critics * c->n_quantiles * n_target);
}

namespace {

#pragma clang fp contract(off)
/* one (row, critic, quantile) of the loss: the two chains over the row's targets */
void qc_huber_chains(float q, const float* t, int nt, float tau, float* lt, float* gs) {
    float a_l = 0.0f, a_g = 0.0f;
    for (int k = 0; k < nt; k++) {
        const float d = t[k] - q;
        const float w = std::fabs(tau - (d < 0.0f ? 1.0f : 0.0f));
        const float ad = std::fabs(d);
        const float huber = ad > 1.0f ? ad - 0.5f : (d * d) * 0.5f;
        const float clamp = d < -1.0f ? -1.0f : (d > 1.0f ? 1.0f : d);
        a_l = std::fmaf(w, huber, a_l);
        a_g = std::fmaf(w, clamp, a_g);
    }
    *lt = a_l;
    *gs = a_g;
}

/* beta ^ step in double by squaring, the lowest bit first */
double pow_by_squaring(double beta, uint64_t step) {
    double p = 1.0, s = beta;
    for (uint64_t n = step; n; n >>= 1) {
        if (n & 1) p = p * s;
        s = s * s;
    }
    return p;
}

void adam_element(float* p, float g, float* m, float* v, float step_size, float c2, float omb1, float b2, float omb2,
                  float eps) {
    *m = *m + (g - *m) * omb1;
    *v = *v * b2 + omb2 * (g * g);
    const float u = step_size * (*m / (std::sqrt(*v) / c2 + eps));
    if (!(u == 0.0f)) *p = *p - u;
}
#pragma clang fp contract(on)

}  // namespace

extern "C" int pgx_qc_critic_grad_host(const pgx_qc_config* cfg, const pgx_qc_weights* w, const pgx_qc_grad_io* io,
                                       int32_t B, int32_t n_target, const pgx_qc_weights* grads) {
    const char* what = "pgx_qc_critic_grad_host";
    int rc = pgx_qc_check_config(cfg, what);
    if (rc == PGX_OK) rc = pgx_qc_check_weights(cfg, w, what);
    if (rc == PGX_OK) rc = pgx_qc_check_grad_launch(cfg, io, B, n_target, what);
    if (rc == PGX_OK) rc = pgx_qc_check_weights(cfg, grads, what);
    if (rc != PGX_OK) return rc;
    const int od = cfg->obs_dim, A = cfg->action_dim, nl = cfg->n_layers, nq = cfg->n_quantiles, nc = cfg->n_critics;
    const int K = od + 6 + A, K16 = up16(K), Q16 = up16(nq), T = nc * nq;
    int sumH = 0, sumH16 = 0;
    for (int l = 0; l < nl; l++) {
        sumH += cfg->hidden[l];
        sumH16 += up16(cfg->hidden[l]);
    }
    const int64_t W = pgx_qc_grad_row_floats(cfg);
    const int CW = 2 * sumH16 + Q16, loss_off = K16 + nc * CW;
    /* workspace columns of critic c: A_l, dZ_l (l = nl: the head's) */
    auto a_off = [&](int c, int l) {
        int o = K16 + c * CW;
        for (int i = 0; i < l; i++) o += up16(cfg->hidden[i]);
        return o;
    };
    auto dz_off = [&](int c, int l) { return a_off(c, l) + sumH16; };
    auto width = [&](int l) { return l < nl ? cfg->hidden[l] : nq; };
    const float inv_count = pgx_qc_inv_count(cfg, B, n_target);
    float* ws = io->workspace;
    for (int32_t b = 0; b < B; b++) {
        float* row = ws + (size_t)b * W;
        for (int64_t i = 0; i < W; i++) row[i] = 0.0f;
        stage_row(row, io, (size_t)b, od, io->action, io->action_stride, A);
        float q[PGX_QC_MAX_QUANTILES];
        float rl = 0.0f;
        for (int c = 0; c < nc; c++) {
            const float* in = row;
            int Kin = K;
            for (int l = 0; l < nl; l++) {
                linear(w->weight[c][l], w->bias[c][l], in, Kin, cfg->hidden[l], true, row + a_off(c, l));
                in = row + a_off(c, l);
                Kin = cfg->hidden[l];
            }
            linear(w->weight[c][nl], w->bias[c][nl], in, Kin, nq, false, q);
            float* dq = row + dz_off(c, nl);
            for (int j = 0; j < nq; j++) {
                const float tau = ((float)j + 0.5f) / (float)nq;
                float lt, gs;
                qc_huber_chains(q[j], io->target_quantiles + (size_t)b * n_target, n_target, tau, &lt, &gs);
                dq[j] = (-inv_count) * gs;
                rl = rl + lt;
                const size_t o = (size_t)b * T + c * nq + j;
                if (io->quantiles_out) io->quantiles_out[o] = q[j];
                if (io->dq_out) io->dq_out[o] = dq[j];
            }
            for (int l = nl; l >= 1; l--) {
                const int out = width(l), O16 = up16(out), Kl = cfg->hidden[l - 1];
                const float* dz = row + dz_off(c, l);
                const float* act = row + a_off(c, l - 1);
                float* dzp = row + dz_off(c, l - 1);
                const float* Wl = w->weight[c][l];
                for (int k = 0; k < Kl; k++) {
                    float acc = 0.0f;
                    for (int o = 0; o < out; o++) acc = std::fmaf(dz[o], Wl[(size_t)o * Kl + k], acc);
                    for (int o = out; o < O16; o++) acc = std::fmaf(0.0f, 0.0f, acc);
                    dzp[k] = act[k] > 0.0f ? acc : 0.0f;
                    if (io->dz_out) {
                        int col = c * sumH + k;
                        for (int i = 0; i < l - 1; i++) col += cfg->hidden[i];
                        io->dz_out[(size_t)b * nc * sumH + col] = dzp[k];
                    }
                }
            }
        }
        row[loss_off] = rl;
    }
    const int B4 = (B + 3) / 4 * 4;
    for (int c = 0; c < nc; c++)
        for (int l = 0; l <= nl; l++) {
            const int out = width(l), in = l == 0 ? K : cfg->hidden[l - 1];
            const int ao = l == 0 ? 0 : a_off(c, l - 1), zo = dz_off(c, l);
            float* dW = const_cast<float*>(grads->weight[c][l]);
            float* db = const_cast<float*>(grads->bias[c][l]);
            for (int o = 0; o < out; o++) {
                for (int k = 0; k < in; k++) {
                    float acc = 0.0f;
                    for (int b = 0; b < B; b++) acc = std::fmaf(ws[(size_t)b * W + zo + o], ws[(size_t)b * W + ao + k], acc);
                    for (int b = B; b < B4; b++) acc = std::fmaf(0.0f, 0.0f, acc);
                    dW[(size_t)o * in + k] = acc;
                }
                float acc = 0.0f;
                for (int b = 0; b < B; b++) acc = std::fmaf(ws[(size_t)b * W + zo + o], 1.0f, acc);
                for (int b = B; b < B4; b++) acc = std::fmaf(0.0f, 0.0f, acc);
                db[o] = acc;
            }
        }
    float total = 0.0f;
    for (int32_t b0 = 0; b0 < B; b0 += 64) {
        float seg = 0.0f;
        for (int32_t b = b0; b < B && b < b0 + 64; b++) seg = seg + ws[(size_t)b * W + loss_off];
        total = total + seg;
    }
    *io->loss = total * inv_count;
    return PGX_OK;
}

extern "C" int pgx_qc_adam_step_host(const pgx_qc_config* cfg, const pgx_qc_weights* params, const pgx_qc_weights* grads,
                                     const pgx_qc_weights* exp_avg, const pgx_qc_weights* exp_avg_sq, uint64_t* step,
                                     double lr, double beta1, double beta2, double eps) {
    const char* what = "pgx_qc_adam_step_host";
    int rc = pgx_qc_check_config(cfg, what);
    if (rc == PGX_OK) rc = pgx_qc_check_adam(beta1, beta2, eps, what);
    for (const pgx_qc_weights* w : {params, grads, exp_avg, exp_avg_sq})
        if (rc == PGX_OK) rc = pgx_qc_check_weights(cfg, w, what);
    if (rc != PGX_OK) return rc;
    if (!step) return bad(what, "null step");
    *step += 1;
    const float bc1 = (float)(1.0 - pow_by_squaring(beta1, *step)), bc2 = (float)(1.0 - pow_by_squaring(beta2, *step));
    const float step_size = (float)lr / bc1, c2 = std::sqrt(bc2);
    const float omb1 = (float)(1.0 - beta1), b2 = (float)beta2, omb2 = (float)(1.0 - beta2), e = (float)eps;
    const int nl = cfg->n_layers, K = cfg->obs_dim + 6 + cfg->action_dim;
    for (int c = 0; c < cfg->n_critics; c++)
        for (int l = 0; l <= nl; l++) {
            const int out = l < nl ? cfg->hidden[l] : cfg->n_quantiles, in = l == 0 ? K : cfg->hidden[l - 1];
            for (int pass = 0; pass < 2; pass++) {
                auto at = [&](const pgx_qc_weights* w) { return const_cast<float*>(pass ? w->bias[c][l] : w->weight[c][l]); };
                float *p = at(params), *g = at(grads), *m = at(exp_avg), *v = at(exp_avg_sq);
                const size_t n = pass ? (size_t)out : (size_t)out * in;
                for (size_t i = 0; i < n; i++) adam_element(p + i, g[i], m + i, v + i, step_size, c2, omb1, b2, omb2, e);
            }
        }
    return PGX_OK;
}
