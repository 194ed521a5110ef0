// hgd_set_tuning: the process-wide tuning keys of hgd.h. The SpMM hop's knobs live here
// (spmm_tuning); the others are set through their owners' set_* functions (hgd_internal.h).
#include "hgd_internal.h"

namespace hgd {

namespace {
SpmmTuning g_spmm;
}

SpmmTuning& spmm_tuning() { return g_spmm; }

}  // namespace hgd

extern "C" hgd_status hgd_set_tuning(int32_t key, int32_t value) {
  using namespace hgd;
  clear_error();
  SpmmTuning& spmm = spmm_tuning();
  switch (key) {
    case HGD_TUNE_SPMM_UNROLL:
      HGD_REQUIRE(value == 8 || value == 16, "hgd_set_tuning: unroll must be 8 or 16");
      spmm.unroll = value;
      return HGD_OK;
    case HGD_TUNE_SPMM_POLICY:
      HGD_REQUIRE(value == 0 || value == 1 || (value >= 8 && value <= 11),
                  "hgd_set_tuning: policy must be 0, 1 (nt stores), 8 (index prefetch), 9, 10 "
                  "(prefetch + nt index loads) or 11");
      spmm.policy = value;
      return HGD_OK;
    case HGD_TUNE_SPMM_PASS_COLS:
      HGD_REQUIRE(value == 0 || value == 64 || value == 128 || value == 256,
                  "hgd_set_tuning: pass columns must be 0 (auto), 64, 128 or 256");
      spmm.pass_cols = value;
      return HGD_OK;
    case HGD_TUNE_ROWGEMM_BLOCKS:
      HGD_REQUIRE(value == 0 || (value >= 64 && value <= 8192),
                  "hgd_set_tuning: row-GEMM blocks must be 0 (default) or in [64, 8192]");
      set_row_gemm_max_blocks(value);
      return HGD_OK;
    case HGD_TUNE_SPLITK_ROWS:
      HGD_REQUIRE(value == 0 || (value >= 64 && value <= 65536 && value % 64 == 0),
                  "hgd_set_tuning: split-K rows must be 0 (default) or a multiple of 64 in "
                  "[64, 65536]");
      set_splitk_rows(value);
      return HGD_OK;
    case HGD_TUNE_GEMM_EXACT:
      HGD_REQUIRE(value == 0 || value == 1, "hgd_set_tuning: gemm exact must be 0 or 1");
      set_gemm_exact(value);
      return HGD_OK;
    case HGD_TUNE_X3_COLS:
      HGD_REQUIRE(value == 0 || value == 64 || value == 128,
                  "hgd_set_tuning: x3 columns must be 0 (default), 64 or 128");
      set_x3_cols(value);
      return HGD_OK;
    case HGD_TUNE_X3_SPLITK:
      HGD_REQUIRE(value >= 0 && value <= 2, "hgd_set_tuning: x3 split-K must be 0, 1 or 2");
      set_x3_splitk(value);
      return HGD_OK;
    case HGD_TUNE_X3S_TILES:
      HGD_REQUIRE(value >= 0 && value <= 3, "hgd_set_tuning: x3s tiles must be 0, 1, 2 or 3");
      set_x3s_tiles(value);
      return HGD_OK;
    case HGD_TUNE_P2P_SEGMENT_MB:
      HGD_REQUIRE(value >= 0 && value <= 65536,
                  "hgd_set_tuning: p2p segment must be 0 (default) or 1..65536 MiB");
      set_p2p_segment_mb(value);
      return HGD_OK;
    case HGD_TUNE_P2P_CACHED:
      HGD_REQUIRE(value == 0 || value == 1, "hgd_set_tuning: p2p cached must be 0 or 1");
      set_p2p_cached(value);
      return HGD_OK;
    case HGD_TUNE_X3P_QUEUE:
      HGD_REQUIRE(value == 0 || value == 1, "hgd_set_tuning: x3p queue must be 0 or 1");
      set_x3p_queue(value);
      return HGD_OK;
    case HGD_TUNE_P2P_GRID:
      HGD_REQUIRE(value >= 0 && value <= 65536, "hgd_set_tuning: p2p grid must be 0..65536");
      set_p2p_grid(value);
      return HGD_OK;
    case HGD_TUNE_MASK_PAIR:
      HGD_REQUIRE(value >= 0 && value <= 2, "hgd_set_tuning: mask pair must be 0, 1 or 2");
      spmm.mask_pair = value;
      return HGD_OK;
    case HGD_TUNE_MASK_DIV:
      HGD_REQUIRE(value == 0 || value == 1, "hgd_set_tuning: mask div must be 0 or 1");
      spmm.mask_div = value;
      return HGD_OK;
    case HGD_TUNE_SPMM_PASS_INTERLEAVE:
      HGD_REQUIRE(value == 0 || value == 1, "hgd_set_tuning: pass interleave must be 0 or 1");
      spmm.pass_interleave = value;
      return HGD_OK;
    case HGD_TUNE_SPMM_BLOCKED_SEG:
      HGD_REQUIRE(value == 0 || value == 1, "hgd_set_tuning: blocked seg must be 0 or 1");
      spmm.blocked_seg = value;
      return HGD_OK;
    case HGD_TUNE_CPU_RNG_THREADS:
      HGD_REQUIRE(value >= 0 && value <= 64, "hgd_set_tuning: cpu rng threads must be 0..64");
      set_cpu_rng_threads(value);
      return HGD_OK;
    default:
      return fail(HGD_ERR_INVALID_ARG, "hgd_set_tuning: unknown key %d", key);
  }
}
