// host_routes_shim.cpp -- C entry points over lz4_flex_amd/csrc/lz4_route.h for tests/test_host_routes.py (ctypes).  Test infrastructure.
#include "../../lz4_flex_amd/csrc/lz4_route.h"

using namespace lz4flex_dev;

extern "C" {

// st: dec_variant, dec_pcd_pair, dec_shared, dec_partial, pair_ws, tools, plan_fits
// sh: n, big_blocks, prefix, chained, chain_prev, n_chains, block_dicts, dict_source, partial
// out: decoder, pcd_geometry, pair, redo (0 none, 1 batch, 2 chain order)
void hr_decode_route(const int* st, const uint32_t* sh, int* out) {
    const DecodeRoute r = decode_route(DecodeSettings{st[0], st[1], st[2], st[3], st[4] != 0, st[5] != 0, st[6] != 0},
                                       DecodeShape{sh[0], sh[1] != 0, sh[2] != 0, sh[3] != 0, sh[4] != 0, sh[5], sh[6] != 0, sh[7] != 0, sh[8] != 0});
    out[0] = r.decoder; out[1] = r.pcd_geometry; out[2] = r.pair ? 1 : 0;
    out[3] = r.redo == Redo::None ? 0 : r.redo == Redo::Batch ? 1 : 2;
}

// st: comp_mode, comp_high_dict, comp_high_linked;  sh: dicts, flags, linked_frame;  out: mode, form (0 plain, 1 dictionary, 2 history)
void hr_encode_route(const int* st, const int* sh, int* out) {
    const EncodeRoute r = encode_route(EncodeSettings{st[0], st[1], st[2]}, EncodeShape{sh[0] != 0, sh[1] != 0, sh[2] != 0});
    out[0] = r.mode;
    out[1] = r.form == HighForm::Plain ? 0 : r.form == HighForm::Dict ? 1 : 2;
}

int hr_variant_ok(int v, int tools) { return decoder_variant(v, tools != 0) != nullptr; }
int hr_decoder_config(int i, int tools) { return decoder_config(i, tools != 0); }
int hr_threshold(int i) { return i >= 0 && i < (int)(sizeof DISPATCH_THRESHOLDS / sizeof DISPATCH_THRESHOLDS[0]) ? (int)DISPATCH_THRESHOLDS[i] : -1; }
uint32_t hr_chain_max_blocks() { return CHAIN_MAX_BLOCKS; }

}  // extern "C"
