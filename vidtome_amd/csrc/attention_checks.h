// The operand checks the attention side exports share (attention_sets.hip, attention_bias.hip, attention_segments.hip,
// attention_probs.hip, attention_words.hip, attention_mass.hip), each stated once, and the dispatch of their launches over
// the two 16-bit types.  Host functions: `who` is the export's name, the answer VTM_OK or what vtm::fail returned, so an
// export keeps the ORDER of its checks with `if (int rc = check_x(who, ...)) return rc;`.  Where one fragment of a message
// differs between the exports it is a parameter; a check only one export makes stays at that export.
// tests/test_attention_contract_host.py pins every message.
#pragma once
#include "attention_plan.h"

#include <cmath>

namespace vtm_att {

inline int check_scale(const char *who, float scale) {
    VTM_REQUIRE(scale > 0.0f && std::isfinite(scale), "%s: scale must be positive and finite", who);
    return VTM_OK;
}

// fp16 / bf16 only; fp32, which the plain core does take, gets a message of its own
inline int check_half_dtype(const char *who, int dtype) {
    if (dtype == VTM_F32)
        return vtm::fail(VTM_EINVAL, "%s: fp32 operands are not taken (dtype must be VTM_F16 or VTM_BF16)", who);
    if (dtype != VTM_F16 && dtype != VTM_BF16) return vtm::fail(VTM_EINVAL, "%s: dtype must be VTM_F16 or VTM_BF16", who);
    return VTM_OK;
}

// fp32 rows with one entry per key, `name` = "bias" (of `noun` "values") or "w" ("weights"): a row holds Mk entries, and
// there is one row for every sample (stride 0) or per-sample rows that do not overlap
inline int check_key_rows(const char *who, const char *name, const char *noun, int64_t ld, int64_t batch_stride, int64_t Mk) {
    VTM_REQUIRE(ld >= Mk, "%s: ld_%s = %lld is shorter than a row of Mk = %lld %s", who, name, (long long)ld, (long long)Mk, noun);
    VTM_REQUIRE(batch_stride == 0 || batch_stride >= ld, "%s: %s_batch_stride = %lld must be 0 or at least ld_%s = %lld", who,
                name, (long long)batch_stride, name, (long long)ld);
    return VTM_OK;
}

// K / V^T tiles are addressed with 32-bit byte offsets inside one (`unit`, head) slice (buffer loads, attention_stage.h)
inline int check_kv_slices(const char *who, const char *unit, int64_t Mkp, int64_t ldk, int64_t d, int64_t ldvt) {
    VTM_REQUIRE((Mkp * ldk + d) * 2 < (1ll << 31) && (d * ldvt + Mkp) * 2 < (1ll << 31),
                "%s: a (%s, head) slice of K or V^T must stay below 2 GiB", who, unit);
    return VTM_OK;
}

// ---- the q / k views of the map exports (vtm_attention_probs, vtm_attention_word_map, vtm_attention_key_mass) ----

// `others_ok`: what the export asks of its other pointers
inline int check_qk_aligned(const char *who, const void *q, const void *k, bool others_ok) {
    VTM_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k)) & 15) == 0 && others_ok,
                "%s: q and k must be 16-byte aligned", who);
    return VTM_OK;
}

inline int check_map_sizes(const char *who, int64_t B, int64_t h, int64_t Mq, int64_t Mqp, int64_t Mk, int64_t Mkp, int64_t d) {
    VTM_REQUIRE(B > 0 && h > 0 && Mq > 0 && Mqp >= Mq && Mk > 0 && Mkp >= Mk && d > 0, "%s: bad sizes", who);
    return VTM_OK;
}

// `ldo_rule` names the bound `ldo_min` on the output's rows ("ldo >= Mk"); then the K half of check_kv_slices
inline int check_qk_rows(const char *who, int64_t ldq, int64_t ldk, int64_t h, int64_t d, int64_t Mk, int64_t ldo,
                         int64_t ldo_min, const char *ldo_rule) {
    VTM_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldq >= h * d && ldk >= h * d && ldo >= ldo_min,
                "%s: ldq and ldk must be multiples of 8 and hold h * d channels, %s", who, ldo_rule);
    VTM_REQUIRE((Mk * ldk + d) * 2 < (1ll << 31), "%s: a (sample, head) slice of K must stay below 2 GiB", who);
    return VTM_OK;
}

// Calls fn(T{}, std::integral_constant<int, D>{}) with T = __half or vtm_bf16 (check_half_dtype has passed) and the head
// dim as with_head_dim: the body names its launch or its family once, as <decltype(t), decltype(dim)::value>.
template <typename Fn>
auto with_half_head_dim(int dtype, int64_t d, Fn &&fn) {
    return with_head_dim(d, [&](auto dim) { return dtype == VTM_F16 ? fn(__half{}, dim) : fn(vtm_bf16{}, dim); });
}

}  // namespace vtm_att
