#pragma once
#include <stdint.h>

#include "../common.h"

namespace pdt {

// The geometry contract of the implicit-GEMM convolutions (conv_fwd.hip), shared by the 16-bit (ConvFwdArgs) and
// the fp32 (Conv32Args) kernels, which derive from it: GEMM row m = (n, i, j) of an N x Pm x Qm sub-grid reads
// input pixel i*ist + ioff + t*tstep for tap t and writes output pixel i*ost + ooff.
struct ConvGeom {
  int N, H, W, C, Kout, T, U;
  int cs;                                              // elements per input pixel.  16-bit kernels: normally == C
                                                       // (the binding fills it); fp32 kernels: 0 means C
  int Pm, Qm;                                          // GEMM-M sub-grid (M = N*Pm*Qm)
  int ist_h, ist_w, ioff_h, ioff_w, tstep_h, tstep_w;  // in = i*ist + ioff + t*tstep
  int OH, OW, ost_h, ost_w, ooff_h, ooff_w;            // out = i*ost + ooff
  int64_t M;                                           // < 2^31 (32-bit fast division of pixel indices)
  // Multi-phase launch (backward-data of strided convs): blockIdx.y selects a phase whose geometry
  // overrides T, U, ioff, Pm, Qm, ooff and the weight offset.  nphase == 0: single-phase launch.
  int nphase;
  int pT[4], pU[4], pioff_h[4], pioff_w[4], pPm[4], pQm[4], pooff_h[4], pooff_w[4];
  int64_t pwoff[4];
  // ---- filled by conv_geom_plan / the launcher
  int m_tiles, n_tiles;
  uint32_t pq_mul, pq_shift, q_mul, q_shift;  // FastDiv by Pm*Qm and Qm
  int pmt[4];                                 // M tiles of each phase
  uint32_t ppq_mul[4], ppq_shift[4], pq1_mul[4], pq1_shift[4];
  float* srows;  // per-block partial statistics rows behind the fp64 slots
  int srows_pp;  // rows per phase (multi-phase launches: row = phase * srows_pp + M tile)

  // the geometry phase p's blocks run with (host side: eligibility predicates of single-phase launches)
  ConvGeom with_phase(int p) const {
    ConvGeom g = *this;
    g.T = pT[p]; g.U = pU[p];
    g.ioff_h = pioff_h[p]; g.ioff_w = pioff_w[p];
    g.Pm = pPm[p]; g.Qm = pQm[p];
    g.ooff_h = pooff_h[p]; g.ooff_w = pooff_w[p];
    g.M = (int64_t)N * g.Pm * g.Qm;
    return g;
  }
};

// Tiles the launch: m_tiles / n_tiles, every FastDiv, the per-phase tile counts and srows_pp.  Returns the number
// of statistics rows (one per (phase, M tile)) and the grid's x size (multi-phase launches: sized for the largest
// phase); *grid_x == 0: nothing to launch.  An empty phase's FastDivs stay unset.
inline int conv_geom_plan(ConvGeom& g, int bm, int bn, int* grid_x) {
  g.m_tiles = (int)((g.M + bm - 1) / bm);
  g.n_tiles = g.Kout / bn;
  const FastDiv f1 = make_fastdiv((uint32_t)(g.Pm * g.Qm)), f2 = make_fastdiv((uint32_t)g.Qm);
  g.pq_mul = f1.mul; g.pq_shift = f1.shift; g.q_mul = f2.mul; g.q_shift = f2.shift;
  int mt = g.m_tiles;
  if (g.nphase > 0) {
    mt = 0;
    for (int p = 0; p < g.nphase; ++p) {
      g.pmt[p] = (int)(((int64_t)g.N * g.pPm[p] * g.pQm[p] + bm - 1) / bm);
      mt = mt > g.pmt[p] ? mt : g.pmt[p];
      if (g.pPm[p] > 0 && g.pQm[p] > 0) {
        const FastDiv p1 = make_fastdiv((uint32_t)(g.pPm[p] * g.pQm[p])), p2 = make_fastdiv((uint32_t)g.pQm[p]);
        g.ppq_mul[p] = p1.mul; g.ppq_shift[p] = p1.shift; g.pq1_mul[p] = p2.mul; g.pq1_shift[p] = p2.shift;
      }
    }
  }
  g.srows_pp = mt;
  *grid_x = mt * g.n_tiles;
  return (g.nphase > 0 ? g.nphase : 1) * mt;
}

#ifdef __HIPCC__
// Multi-phase launch: overwrite ``a`` (the kernel's private copy of its arguments ``args``) with phase ph's geometry
// (wave-uniform), the weights at wbase + the phase's offset.  Returns whether blockIdx.x is one of the phase's tiles:
// the grid is sized for the largest phase, and a block beyond its own phase's tiles has to zero the statistics row
// it owns and return.  ``args`` itself is only read: a write makes the compiler copy the kernel-argument struct,
// with its dynamically indexed phase arrays, to scratch (see conv_fwd_kernel).
template <class Args, class WT>
PDT_DEVICE bool select_phase(Args& a, const Args& args, const WT* wbase, int ph) {
  a.T = args.pT[ph]; a.U = args.pU[ph];
  a.ioff_h = args.pioff_h[ph]; a.ioff_w = args.pioff_w[ph];
  a.Pm = args.pPm[ph]; a.Qm = args.pQm[ph];
  a.ooff_h = args.pooff_h[ph]; a.ooff_w = args.pooff_w[ph];
  a.m_tiles = args.pmt[ph];
  a.M = (int64_t)a.N * a.Pm * a.Qm;
  a.w = wbase + args.pwoff[ph];
  a.pq_mul = args.ppq_mul[ph]; a.pq_shift = args.ppq_shift[ph];
  a.q_mul = args.pq1_mul[ph]; a.q_shift = args.pq1_shift[ph];
  return (int)blockIdx.x < a.m_tiles * a.n_tiles;
}
#endif

}  // namespace pdt
