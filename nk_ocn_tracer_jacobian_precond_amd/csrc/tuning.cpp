// The part of the C ABI that needs no device: default options, tuning knobs (defaults, environment, validation) and the calling
// thread's error message.  Plain C++, no HIP: the host-only units (dist_plan.cpp, ml_plan.cpp) link against it alone.
#include "tuning.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static thread_local std::string g_last_error;

int fail (int code, const char *fmt, ...)
{
   char buf[512];
   va_list ap;
   va_start (ap, fmt);
   vsnprintf (buf, sizeof buf, fmt, ap);
   va_end (ap);
   g_last_error = buf;
   return code;
}

extern "C" const char *nkp_last_error (void) { return g_last_error.c_str (); }
std::string last_error_message () { return g_last_error; }
void restore_error_message (const std::string &text) { g_last_error = text; }

extern "C" int nkp_default_options (nkp_options *opt)
{
   if (!opt) return NKP_EINVAL;
   memset (opt, 0, sizeof *opt);
   opt->struct_size = (int) sizeof (nkp_options);
   opt->precond = NKP_PRECOND_MULTILEVEL;
   opt->krylov = NKP_KRYLOV_FGMRES;
   opt->restart = 200;
   opt->max_iters = 20000;
   opt->rtol = 1.0e-10;
   opt->atol = 0.0;
   opt->device = -1;
   opt->verbose = 0;
   opt->rank = 0;
   opt->reorth = 0;
   opt->ml_levels = 0;
   opt->ml_smooth = 3;
   opt->precond_steps = 0;   // automatic
   opt->equil = 0;           // automatic
   opt->basis_f32 = 0;       // f32 basis: -11 % time at 1 degree, but it doubled the iterations of the 3 degree solve with one Gram-Schmidt pass
   return NKP_OK;
}

// ---------------------------------------------------------------- tuning knobs (include/nkp.h: nkp_tuning)
static void builtin_tuning (nkp_tuning *t)
{
   memset (t, 0, sizeof *t);
   t->struct_size = (int) sizeof (nkp_tuning);
   t->ml_split = 1; t->ml_pocket = 4; t->ml_big_from = -3; t->ml_coarsest_rows = 8000; t->ml_dense_max = 8192;
   t->ml_theta = 0.0; t->ml_tau = 0.01; t->ml_device_min = 100000;
   t->ml_smooth_coarse = 0; t->ml_coarse_from = 2; t->ml_gamma_from = 0; t->ml_gamma_to = 0; t->ml_f32 = 1; t->ml_host_inverse = 0;
   t->ml_fused = 0; t->ml_fused_max_cols = 0; t->ml_wave_fused = 1; t->ml_coarsest_sweeps = 30; t->ml_tail_rows = 0; t->ml_omega = 1.1;
   t->col_ldsres = 2; t->col_stream = 1; t->col_stream_min = -1; t->col_stream_gw = 32; t->col_wave_max = 8192; t->col_w3 = 1;
   t->col_group = 8; t->col_pipe_min = 0; t->col_ldsres_early = 0; t->col_ldsres_packed = 1; t->col_sort_groups = 1;
   t->spmv_variant = 4; t->spmv_compress = 0; t->spmv_pipe_min = 1024; t->spmv_run = 1; t->spmv_wgs = 256;
   t->rhs_batch = 1; t->batch_spmv_rows = 1; t->precond_steps = 0; t->equil = -1; t->dist_overlap = 1; t->dist_ras = 1; t->dist_one_reduce = 0; t->force_dist = 0; t->setup_threads = 0; t->plan_times = 0;
   t->ml_drop_intertracer = 0; t->ml_huge_from = -1; t->dist_ras_rings = 1; t->ml_diag = 32; t->spmv_diag = 32;
   t->ml_lane_fused = 50000; t->dist_smooth_exchange = 0; t->step_glue = 12;
}

const nkp_tuning &nkp_builtin_tuning ()
{
   static const nkp_tuning t = [] { nkp_tuning q; builtin_tuning (&q); return q; } ();
   return t;
}

extern "C" int nkp_default_tuning (nkp_tuning *t)
{
   if (!t) return NKP_EINVAL;
   builtin_tuning (t);
   const char *e;
#define ENV_INT(name, field) do { if ((e = getenv (name)) && *e) t->field = atoi (e); } while (0)
#define ENV_POS(name, field) do { if ((e = getenv (name)) && atoi (e) > 0) t->field = atoi (e); } while (0)
#define ENV_FLAG(name, field) do { if ((e = getenv (name)) && *e) t->field = atoi (e) != 0; } while (0)
   ENV_FLAG ("NKP_ML_SPLIT", ml_split); ENV_INT ("NKP_ML_POCKET", ml_pocket); ENV_INT ("NKP_ML_BIG_FROM", ml_big_from);
   ENV_INT ("NKP_ML_COARSEST_ROWS", ml_coarsest_rows); ENV_INT ("NKP_ML_DENSE_MAX", ml_dense_max);
   if ((e = getenv ("NKP_ML_THETA")) && *e) t->ml_theta = atof (e);
   if ((e = getenv ("NKP_ML_TAU")) && *e) t->ml_tau = atof (e);
   if ((e = getenv ("NKP_ML_DEVICE_MIN")) && *e) t->ml_device_min = atoll (e);
   ENV_POS ("NKP_ML_SMOOTH_COARSE", ml_smooth_coarse); ENV_POS ("NKP_ML_COARSE_FROM", ml_coarse_from);
   ENV_INT ("NKP_ML_GAMMA_FROM", ml_gamma_from); ENV_INT ("NKP_ML_GAMMA_TO", ml_gamma_to);
   ENV_FLAG ("NKP_ML_F32", ml_f32); ENV_FLAG ("NKP_ML_HOST_INVERSE", ml_host_inverse); ENV_FLAG ("NKP_ML_FUSED", ml_fused);
   ENV_INT ("NKP_ML_FUSED_MAX_COLS", ml_fused_max_cols); ENV_INT ("NKP_ML_WAVE_FUSED", ml_wave_fused); ENV_POS ("NKP_ML_COARSEST_SWEEPS", ml_coarsest_sweeps);
   if ((e = getenv ("NKP_ML_TAIL_ROWS")) && *e) t->ml_tail_rows = atoll (e);
   if ((e = getenv ("NKP_ML_OMEGA")) && atof (e) > 0.0) t->ml_omega = atof (e);
   ENV_INT ("NKP_COL_LDSRES", col_ldsres); ENV_FLAG ("NKP_COLSTREAM", col_stream); ENV_INT ("NKP_COLSTREAM_MIN", col_stream_min);
   if ((e = getenv ("NKP_COLSTREAM_GW")) && *e) t->col_stream_gw = atoi (e) == 64 ? 64 : 32;
   ENV_INT ("NKP_COLWAVE_MAX", col_wave_max); ENV_FLAG ("NKP_COL_W3", col_w3); ENV_INT ("NKP_COLGROUP", col_group);
   ENV_INT ("NKP_COLPIPE_MIN", col_pipe_min); ENV_FLAG ("NKP_LDSRES_EARLY", col_ldsres_early); ENV_FLAG ("NKP_COL_PACKED", col_ldsres_packed); ENV_FLAG ("NKP_COL_SORT_GROUPS", col_sort_groups); ENV_INT ("NKP_COL_LDSRES_MIN", col_ldsres_min); ENV_INT ("NKP_ML_HUGE_FROM", ml_huge_from);
   ENV_INT ("NKP_SPMV_VARIANT", spmv_variant); ENV_FLAG ("NKP_SPMV_COMPRESS", spmv_compress); ENV_INT ("NKP_SPMV_PIPE_MIN", spmv_pipe_min);
   ENV_POS ("NKP_SPMV_RUN", spmv_run); ENV_POS ("NKP_SPMV_WGS", spmv_wgs);
   ENV_INT ("NKP_RHS_BATCH", rhs_batch); ENV_FLAG ("NKP_BATCH_SPMV_ROWS", batch_spmv_rows);
   ENV_POS ("NKP_PRECOND_STEPS", precond_steps); ENV_FLAG ("NKP_EQUIL", equil);
   ENV_FLAG ("NKP_DIST_OVERLAP", dist_overlap); ENV_FLAG ("NKP_DIST_RAS", dist_ras); ENV_FLAG ("NKP_DIST_ONE_REDUCE", dist_one_reduce);
   if (getenv ("NKP_FORCE_DIST")) t->force_dist = 1;
   ENV_POS ("NKP_SETUP_THREADS", setup_threads);
   if (getenv ("NKP_ML_PLAN_TIMES")) t->plan_times = 1;
   ENV_FLAG ("NKP_ML_DROP_INTERTRACER", ml_drop_intertracer);
   ENV_INT ("NKP_DIST_RAS_RINGS", dist_ras_rings);
   ENV_INT ("NKP_ML_DIAG", ml_diag);
   ENV_INT ("NKP_SPMV_DIAG", spmv_diag);
   ENV_INT ("NKP_ML_LANE_FUSED", ml_lane_fused);
   ENV_INT ("NKP_DIST_SMOOTH_EXCHANGE", dist_smooth_exchange);
   ENV_INT ("NKP_STEP_GLUE", step_glue);
#undef ENV_INT
#undef ENV_POS
#undef ENV_FLAG
   if (t->spmv_variant < 0 || t->spmv_variant > 9) t->spmv_variant = 4;      // 0-4 stream flavours (5-8: ablation library), 9 rows kernel
   return NKP_OK;
}

// the caller's knobs, or the defaults + environment (the one place a solver looks at the environment); *range_error tells a
// value out of range (out is filled) from a struct of the wrong size (out is not)
int resolve_tuning (const nkp_options *opt, nkp_tuning *out, bool *range_error)
{
   if (range_error) *range_error = false;
   if (opt && opt->tuning) {
      if (opt->tuning->struct_size != (int) sizeof (nkp_tuning)) return fail (NKP_EINVAL, "nkp_tuning.struct_size mismatch (%d != %zu)", opt->tuning->struct_size, sizeof (nkp_tuning));
      *out = *opt->tuning;
   } else {
      const int rc = nkp_default_tuning (out);
      if (rc) return rc;
   }
   if (out->dist_ras_rings < 0 || out->dist_ras_rings > 4) {
      if (range_error) *range_error = true;
      return fail (NKP_EINVAL, "nkp_tuning.dist_ras_rings = %d is out of range (0 = default, 1 .. 4 rings)", out->dist_ras_rings);
   }
   if (out->dist_smooth_exchange != 0 && out->dist_smooth_exchange != 1) {
      if (range_error) *range_error = true;
      return fail (NKP_EINVAL, "nkp_tuning.dist_smooth_exchange = %d is out of range (0 = off, 1 = on)", out->dist_smooth_exchange);
   }
   return NKP_OK;
}
