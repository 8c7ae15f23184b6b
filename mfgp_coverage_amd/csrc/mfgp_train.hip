// Training on the device: the negative log marginal likelihood and its analytic
// gradient (mfgp_nlml.hip) for one hyperparameter vector (mfgp_nlml) and for a batch
// of them over one data set (mfgp_nlml_batch).
#include <cmath>
#include <cstring>

#include "mfgp_host.h"

using namespace mfgp;
using namespace mfgp_host;

namespace {

// The host finish of mfgp_nlml and of every member of mfgp_nlml_batch (one copy, so
// that a member's bits are the single call's): the value from v = (sum log L_ii,
// |z|^2), the gradient from the np tile partials hp (summed in tile order) and the
// mean terms a^T dr/dh from ha = K^-1 r (summed in row order).
void nlml_finish(const mfgp_model* m, const double* hyp, int64_t N, const double* v, const double* hp, int64_t np,
                 const double* ha, double* nlml, double* grad) {
  const int nhyp = m->nhyp;
  // NLML = 1/2 r^T K^-1 r + sum log L_ii + N/2 log(2 pi)   (gp:104-105 / gp:383-384)
  *nlml = 0.5 * v[1] + v[0] + 0.5 * std::log(2.0 * M_PI) * (double)N;
  if (grad) {
    for (int p = 0; p < nhyp; ++p) grad[p] = 0.0;
    const int64_t ntiles = np / 9;
    double g9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t tt = 0; tt < ntiles; ++tt)
      for (int p = 0; p < 9; ++p) g9[p] += hp[tt * 9 + p];
    // mean terms a^T dr/dh (r = y - m(hyp), gp:89-90 / gp:415-424)
    const Hyp h = derive_hyp(m->kind, hyp, m->jitter);
    double sa_lo = 0.0, sa_hi = 0.0;
    for (int64_t i = 0; i < N; ++i) (i < m->NL ? sa_lo : sa_hi) += ha[i];
    if (m->kind == MFGP_SF) {
      grad[0] = -h.meanL * (sa_lo + sa_hi);
      grad[1] = g9[1];
      grad[2] = g9[2];
      grad[3] = g9[3];
    } else {
      for (int p = 0; p < 9; ++p) grad[p] = g9[p];
      grad[0] += -h.meanL * sa_lo - h.rho * h.meanL * sa_hi;
      grad[3] += -std::exp(hyp[3]) * sa_hi;
      grad[6] += -h.rho * h.meanL * sa_hi;
    }
  }
}

// ---- mfgp_nlml_batch: the context's scratch for a chunk of C members of leading
// dimension ld (doubles, member-major inside each array):
//   A [C][ld^2] | Linv [C][ld/64][TILE] | zv [C][ld] | val [C][2] | status [C] (ints)
//   and with the gradient  Xi [C][ld^2] | Kv [C][ld^2] | alpha [C][ld] | part [C][np]
// The pinned host image holds val | part | alpha of a chunk.
struct NlmlLayout {
  int64_t ld, np, C;
  bool grad;
  int64_t o_A, o_Li, o_zv, o_val, o_st, o_Xi, o_Kv, o_al, o_part, total;   // device offsets (doubles)
  int64_t h_val, h_part, h_al, h_total;                                    // host offsets (doubles)
};
int64_t nlml_member_bytes(int64_t ld, int64_t np, bool grad) {
  int64_t n = ld * ld + (ld / NB) * TILE + ld + 2 + 1;
  if (grad) n += 2 * ld * ld + ld + np;
  return n * (int64_t)sizeof(double);
}
NlmlLayout nlml_layout(int64_t ld, int64_t np, int64_t C, bool grad) {
  NlmlLayout l{};
  l.ld = ld;
  l.np = np;
  l.C = C;
  l.grad = grad;
  l.o_A = 0;
  l.o_Li = l.o_A + C * ld * ld;
  l.o_zv = l.o_Li + C * (ld / NB) * TILE;
  l.o_val = l.o_zv + C * ld;
  l.o_st = l.o_val + 2 * C;
  l.o_Xi = round_up(l.o_st + (C + 1) / 2, NB);   // (the tile loads of Xi / Kv are 16-byte ones)
  l.o_Kv = l.o_Xi + (grad ? C * ld * ld : 0);
  l.o_al = l.o_Kv + (grad ? C * ld * ld : 0);
  l.o_part = l.o_al + (grad ? C * ld : 0);
  l.total = l.o_part + (grad ? C * np : 0);
  l.h_val = 0;
  l.h_part = 2 * C;
  l.h_al = l.h_part + (grad ? C * np : 0);
  l.h_total = l.h_al + (grad ? C * ld : 0);
  return l;
}
int ensure_nlml_scratch(mfgp_ctx* c, const NlmlLayout& l) {
  const size_t dev = sizeof(double) * (size_t)l.total, host = sizeof(double) * (size_t)l.h_total;
  int rc;
  if (dev > c->nb_dev.bytes() && (rc = dev_alloc(c->nb_dev, c->stream, dev))) return rc;
  if (host > c->nb_host.bytes()) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    if ((rc = pin_alloc(c->nb_host, host, hipHostMallocDefault))) return rc;
  }
  return MFGP_OK;
}
}  // namespace

extern "C" {

// likelihood (gp:81-106 / gp:344-385) and its analytic gradient on the device,
// for the model's data under the given hyperparameters (the model is unchanged).
int mfgp_nlml(mfgp_model* m, const double* hyp, int nhyp, double* nlml, double* grad) {
  const Entry entry(m);
  int rc = entry.rc;
  if (rc) return rc;
  if (!hyp || nhyp != m->nhyp)
    return set_err(MFGP_ERR_ARG, "Hyperparameters must be of length 4 (single-fidelity) or 9 (multi-fidelity)");
  if (!nlml) return set_err(MFGP_ERR_ARG, "null output");
  mfgp_ctx* c = m->ctx;
  const int64_t N = m->NL + m->NH;
  if (N == 0) {   // empty data: every term is an empty sum
    *nlml = 0.0;
    if (grad)
      for (int p = 0; p < nhyp; ++p) grad[p] = 0.0;
    return MFGP_OK;
  }
  // scratch factor of K(hyp) and the kernels' scratch: all of it goes on every return
  mfgp_model* t = nullptr;
  if ((rc = mfgp_model_create(c, m->kind, MFGP_F64, hyp, nhyp, m->jitter, &t))) return rc;
  const ModelGuard scratch(t);
  Dev<double> Xi, Kv, al, part, val;
  if ((rc = ensure_cap(t, N))) return rc;
  HIP_TRY(hipMemcpyAsync(t->X, m->X, sizeof(double) * 2 * N, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(t->y, m->y, sizeof(double) * N, hipMemcpyDeviceToDevice, c->stream));
  t->NL = m->NL;
  t->NH = m->NH;
  if ((rc = factor_one(t))) return rc;   // LinAlgError as the reference's cholesky (gp:101 / 380)
  int slot;
  GPDesc* hd = acquire_slot(c, slot, rc);
  if (!hd) return rc;
  fill_desc(hd[0], t);
  const GPDesc* dd = nullptr;
  if ((rc = upload_slot(c, slot, 1, &dd))) return rc;
  if ((rc = dev_alloc(val, c->stream, sizeof(double) * 2, A_NO_DRAIN))) return rc;
  if (launch_nlml_value(dd, 1, val, c->stream) != hipSuccess) return set_err(MFGP_ERR_DEVICE, "launch");
  const int64_t ld = t->ld, np = nlml_partials(N);
  if (grad) {
    if ((rc = dev_alloc(Xi, c->stream, sizeof(double) * ld * ld, A_NO_DRAIN)) ||
        (rc = dev_alloc(Kv, c->stream, sizeof(double) * ld * ld, A_NO_DRAIN)) ||
        (rc = dev_alloc(al, c->stream, sizeof(double) * ld, A_NO_DRAIN)) ||
        (rc = dev_alloc(part, c->stream, sizeof(double) * np, A_NO_DRAIN)))
      return rc;
    if (launch_nlml_grad(dd, N, Xi, Kv, al, part, c->stream) != hipSuccess)
      return set_err(MFGP_ERR_DEVICE, "nlml: launch failed");
  }
  if ((rc = release_slot(c, slot))) return rc;
  double v[2] = {0.0, 0.0};
  std::vector<double> hp, ha;
  HIP_TRY(hipMemcpyAsync(v, val, sizeof(v), hipMemcpyDeviceToHost, c->stream));
  if (grad) {
    hp.resize(np);
    ha.resize(N);
    HIP_TRY(hipMemcpyAsync(hp.data(), part, sizeof(double) * np, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(ha.data(), al, sizeof(double) * N, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  nlml_finish(m, hyp, N, v, hp.data(), np, ha.data(), nlml, grad);
  return MFGP_OK;
}

// mfgp_nlml for S hyperparameter vectors in chunks of C members: per chunk one
// batched factor (enqueue_factor), one read of the members' status words, one launch
// each of k_nlml_value and the four gradient kernels, one synchronisation. The
// members are scratch factors in the context's scratch that read the caller's X / y
// in place; the caller's model is not written.
int mfgp_nlml_batch(mfgp_model* m, const double* hyps, int S, int nhyp, double* nlml, double* grad, int* status) {
  const Entry entry(m);
  int rc = entry.rc;
  if (rc) return rc;
  if (nhyp != m->nhyp)
    return set_err(MFGP_ERR_ARG, "Hyperparameters must be of length 4 (single-fidelity) or 9 (multi-fidelity)");
  if (S < 0) return set_err(MFGP_ERR_ARG, "S must be >= 0");
  if (S == 0) return MFGP_OK;
  if (!hyps) return set_err(MFGP_ERR_ARG, "null hyps");
  if (!nlml) return set_err(MFGP_ERR_ARG, "null output");
  mfgp_ctx* c = m->ctx;
  const int64_t N = m->NL + m->NH;
  if (N == 0) {   // empty data: every term is an empty sum
    for (int s = 0; s < S; ++s) nlml[s] = 0.0;
    if (grad)
      for (int64_t e = 0; e < (int64_t)S * nhyp; ++e) grad[e] = 0.0;
    if (status)
      for (int s = 0; s < S; ++s) status[s] = 0;
    return MFGP_OK;
  }
  // the leading dimension of mfgp_nlml's scratch model (ensure_cap of N rows)
  const int64_t ld = round_up(std::max<int64_t>(N, 63) + 1, NB), np = nlml_partials(N);
  const int64_t per = nlml_member_bytes(ld, np, grad != nullptr);
  int64_t C = c->nlml_chunk > 0 ? c->nlml_chunk : std::max<int64_t>(1, (int64_t)NLML_BATCH_SCRATCH / per);
  C = std::min<int64_t>({C, MAXB, S});
  const NlmlLayout l = nlml_layout(ld, np, C, grad != nullptr);
  if ((rc = ensure_nlml_scratch(c, l))) return rc;
  if ((rc = ensure_h_status(c, (size_t)C))) return rc;
  double* const dv = c->nb_dev;
  int* const dst = reinterpret_cast<int*>(dv + l.o_st);
  const double* const hb = c->nb_host;
  const double nan = std::nan("");
  int first_bad = 0;
  for (int s0 = 0; s0 < S; s0 += (int)C) {
    const int cnt = (int)std::min<int64_t>(C, S - s0);
    int slot;
    GPDesc* hd = acquire_slot(c, slot, rc);
    if (!hd) return rc;
    for (int i = 0; i < cnt; ++i) {
      // a scratch factor of K(hyps[s0 + i]) over the caller's rows: the descriptor fill_desc
      // gives a model without grid, V or scratch (nothing here is owned by a model)
      GPDesc& d = hd[i];
      d = GPDesc{};
      d.X = m->X;
      d.y = m->y;
      d.A = dv + l.o_A + (int64_t)i * ld * ld;
      d.Linv = dv + l.o_Li + (int64_t)i * (ld / NB) * TILE;
      d.zv = dv + l.o_zv + (int64_t)i * ld;
      d.status = dst + i;
      d.rsplit = 1;
      d.ld = ld;
      d.N = N;
      d.NL = m->NL;
      d.ka = 8;
      d.ksplit = 1;
      d.hf = derive_hyp(m->kind, hyps + (size_t)(s0 + i) * nhyp, m->jitter);
      d.hp = d.hf;
    }
    const GPDesc* dd = nullptr;
    if ((rc = upload_slot(c, slot, cnt, &dd))) return rc;
    if ((rc = enqueue_factor(c, dd, hd, cnt))) return rc;
    HIP_TRY(hipMemcpyAsync(c->h_status, dst, sizeof(int) * cnt, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(launch_nlml_value(dd, cnt, dv + l.o_val, c->stream));
    if (grad)
      HIP_TRY(launch_nlml_grad_batch(dd, cnt, N, dv + l.o_Xi, dv + l.o_Kv, dv + l.o_al, dv + l.o_part, ld * ld, ld, np,
                                     c->stream));
    if ((rc = release_slot(c, slot))) return rc;
    HIP_TRY(hipMemcpyAsync(c->nb_host + l.h_val, dv + l.o_val, sizeof(double) * 2 * cnt, hipMemcpyDeviceToHost,
                           c->stream));
    if (grad) {
      HIP_TRY(hipMemcpyAsync(c->nb_host + l.h_part, dv + l.o_part, sizeof(double) * np * cnt, hipMemcpyDeviceToHost,
                             c->stream));
      HIP_TRY(hipMemcpyAsync(c->nb_host + l.h_al, dv + l.o_al, sizeof(double) * ld * cnt, hipMemcpyDeviceToHost,
                             c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < cnt; ++i) {
      const int s = s0 + i, st = c->h_status[i];
      double* const g = grad ? grad + (size_t)s * nhyp : nullptr;
      if (st == INT_MAX) {
        nlml_finish(m, hyps + (size_t)s * nhyp, N, hb + l.h_val + 2 * i, hb + l.h_part + (int64_t)i * np, np,
                    hb + l.h_al + (int64_t)i * ld, nlml + s, g);
        if (status) status[s] = 0;
        continue;
      }
      if (st <= 0) return status_error(st);   // (no order of a leading minor: a device failure)
      // not positive definite (the reference's cholesky raising, gp:101 / 380): this member only
      nlml[s] = nan;
      if (g)
        for (int p = 0; p < nhyp; ++p) g[p] = nan;
      if (status) status[s] = st;
      if (!first_bad) first_bad = st;
    }
  }
  if (!status && first_bad) return status_error(first_bad);
  return MFGP_OK;
}

}  // extern "C"
