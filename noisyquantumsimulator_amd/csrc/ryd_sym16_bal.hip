// ryd_sym16_bal.hip -- the CU-balanced sym16 LP-square kernels (ryd_sym16.inc, BAL = 1, 2 and
// their summary-only twins) in a translation unit of their own.
//
// The Makefile compiles this file with -mllvm -amdgpu-kernarg-preload-count=8: the kernels'
// first eight arguments (14 dwords, all the user SGPRs there are beside the argument pointer)
// arrive in SGPRs at wave entry instead of through s_load.  The option acts on every kernel of
// a translation unit, which is why these four have one to themselves: the rest of the engine,
// the one-wave sym16 kernels included, keeps its code byte for byte.  The device code comes
// from ryd_engine.hip up to ryd_sym16.inc (RYD_S16_BAL_TU ends that file there); only the
// templates instantiated below are emitted.
#define RYD_S16_BAL_TU 1
#include "ryd_engine.hip"

hipError_t ryd_s16_bal_launch(int form, bool state, unsigned workgroups, unsigned block, hipStream_t stream,
                              const double* prm, int64_t n, int64_t ldp, int cfg, double* sm, uint32_t* status,
                              int64_t ldm, double* st, int64_t lds, int n_steps) {
  constexpr int P = RYD_PROTO_LP_SQUARE;
  void (*k)(RYD_S16_BAL_PARAMS) =
      state ? (form == 2 ? lindblad_sym16_kernel<P, 2> : lindblad_sym16_kernel<P, 1>)
            : (form == 2 ? lindblad_sym16_nostate_kernel<P, 2> : lindblad_sym16_nostate_kernel<P, 1>);
  int nwg = (int)workgroups;
  // in the order of RYD_S16_BAL_PARAMS
  void* args[] = {&prm, &n, &ldp, &cfg, &nwg, &sm, &status, &ldm, &st, &lds, &n_steps};
  return hipLaunchKernel((const void*)k, dim3(workgroups), dim3(block), args, 0, stream);
}
