// forms.h -- the kernel forms of the dispatch: their codes, the rule that picks one, and the record of the ones enqueued ("The form record")
// The assign pass is a family of template instantiations picked by table form, stride, launch size and mode, and k_preempt_update has two
// forms.  A form is stated once, as a row (code, kernel) of the tables beside the kernels (assign.hip, preempt.hip); choose_form() below is
// the one rule that picks an assign form, a pure function of a few plain inputs.  Every launch notes the code of the row it took; the
// process keeps the set of distinct codes (fslic_hip_debug_forms_seen) next to the complete list (fslic_hip_debug_forms_all: the rows'
// codes).  Host only: one uncontended mutex per launch, nothing on the device.
#pragma once
#include <cstddef>
#include <cstdint>

namespace fslic {

enum : uint32_t { kFormBlk = 1, kFormBin = 2, kFormPre = 3, kFormK32 = 4, kFormGeneric = 5, kFormGenericRec = 6, kFormPreemptUpdate = 7 };
// which spatial table the launch reads: the row-vector table (`tab` in the full pass, `tabs` in a fused one), the full pass's shorter
// 16-row one (`tabv16`), the 2-D table (`tab` / `tabs`), the subsampled stride's 2-D table for 16 rows (`tabs16`), the 32-bit kernel's LUT
enum : uint32_t { kFormTabNone = 0, kFormTabRowvec = 1, kFormTabRowvec16 = 2, kFormTab2d = 3, kFormTab2d16 = 4, kFormTabLut = 5 };

// bits 0-3 family | 4-9 rows per wavefront | 10 fused | 11-13 stride template (0: run-time argument) | 14-16 table | 17 label-free |
// 18 all-pairs (k_preempt_update); _binding.py decodes the same layout
constexpr uint32_t form_code(uint32_t family, int rows, bool fused, int stride_t, uint32_t table, bool nolab = false, bool all_pairs = false) {
    return family | (uint32_t)rows << 4 | (fused ? 1u : 0u) << 10 | (uint32_t)stride_t << 11 | table << 14 | (nolab ? 1u : 0u) << 17 | (all_pairs ? 1u : 0u) << 18;
}
constexpr uint32_t form_family(uint32_t code) { return code & 15u; }
constexpr int form_rows(uint32_t code) { return (int)(code >> 4 & 63u); }
constexpr bool form_fused(uint32_t code) { return (code >> 10 & 1u) != 0; }
constexpr uint32_t form_table(uint32_t code) { return code >> 14 & 7u; }
constexpr uint32_t kFormNone = 0;      // no form: the entry does not take this geometry (choose_form)

// The launch sizes at which the choice changes, in eight-row assign blocks (assign_blocks8, kernels.h).
constexpr int kBlocksBinRows4 = 384;       // cluster pass fused in, 2-D table, stride 3: up to here 4 rows per wavefront.  Launches that leave most
                                           // of the chip idle even with 8-row wavefronts (one or two 1280x720 frames: 160 blocks each on 256 CUs): a
                                           // wavefront alone on its SIMD issues a dependent instruction every 8 - 10 clocks, so a block's life there
                                           // is its instruction chain; half the rows halve the argmin, label and sum phases of that chain
                                           // (measured: one 1280x720 frame per group 179.5 -> 175.7 us, profiles/r04_assign_experiments.txt)
constexpr int kBlocksFuseBin = 640;        // up to here the cluster pass rides on the assign launches (FSLIC_FUSEBIN=1; group.cpp, cluster_pass_fused)
constexpr int kBlocksRows16Tab2d = 2048;   // fused pass on the 2-D table: beyond, 16 rows per wavefront where `tabs16` exists (the launch then is one
                                           // round of blocks instead of one and a bit)
constexpr int kBlocksRows16 = 3072;        // beyond: 16 rows per wavefront (the full pass; a fused pass on the row-vector table).  Launches of many
                                           // blocks (3840x2160 frames in groups): the block prologue (candidate list, table) is paid once per 4096 pixels
                                           // instead of once per half as many.  Small launches keep 8 rows (more, shorter-lived blocks fill the chip
                                           // better); so does the 2-D table below its own size, whose LDS footprint grows with the rows a wavefront spans
constexpr int kBlocksRows32 = 4 * 6144;    // beyond: 32 rows (full pass, 32-row row-vector table only) -- launches that keep the chip busy for three
                                           // rounds of 16-row blocks and more pay the block prologue and the per-candidate fetch once per 8192 pixels

// What a launch function is asked for ..
enum FormEntry : int {
    kEntryFull,             // launch_assign without the update (the pass that writes the final labels)
    kEntryFused,            // launch_assign with the fused update
    kEntryFusedBin,         // launch_assign_fused_bin: the caller has asked blk_kernel_applies (group.cpp, cluster_pass_fused)
    kEntryPre,              // launch_assign_pre
    kEntryGenericFull, kEntryGenericFused, kEntryGenericRec,      // launch_assign_generic
    kFormEntries
};
// .. and everything the choice depends on (of FrameDev: the tables tables.cpp built)
struct FormInputs {
    int entry;
    bool blk_applies;                  // blk_kernel_applies(f, stride)
    bool tab_vmode, tab_rows32;        // row-vector tables (else 2-D); `tab` built for 32 rows
    bool has_tabs16, has_tabv16, has_lut;
    int stride;
    bool label_free;
    int blocks8;                       // assign_blocks8 of the launch
};

// The form a launch takes.  kFormNone: preemptive mode on a geometry outside the block kernel (launch_assign_pre returns false).  Not
// produced because they do not exist: k_assign with 16 rows and the update (16 rows are the full pass's), 32 rows on anything but the
// 32-row row-vector table.  Every form is chosen together with a guard on the table it reads: none is selected with a table that was not built.
constexpr uint32_t choose_form(const FormInputs& in) {
    const int stride_t = in.stride <= 1 ? 1 : in.stride == 2 ? 2 : 3;      // (the block kernel's strides are 1 .. 3: blk_kernel_applies)
    const uint32_t subsampled = in.tab_vmode ? kFormTabRowvec : kFormTab2d;
    const uint32_t lut = in.has_lut ? kFormTabLut : kFormTabNone;
    switch (in.entry) {
    case kEntryFull:
        if (in.blk_applies && in.stride == 1) {
            const int rows = in.tab_vmode && in.tab_rows32 && in.blocks8 > kBlocksRows32 ? 32 : in.blocks8 > kBlocksRows16 ? 16 : 8;
            // row-vector mode with at most 16 rows per wavefront: the shorter stride-1 table (48 entries = 768 bytes of LDS per block less)
            const uint32_t table = !in.tab_vmode ? kFormTab2d : rows <= 16 && in.has_tabv16 ? kFormTabRowvec16 : kFormTabRowvec;
            return form_code(kFormBlk, rows, false, 1, table, in.label_free);
        }
        return form_code(kFormK32, in.blocks8 > kBlocksRows16 ? 16 : 8, false, 0, lut);
    case kEntryFused:
        if (in.blk_applies) {
            const bool r16 = in.tab_vmode ? in.blocks8 > kBlocksRows16 : in.has_tabs16 && in.blocks8 > kBlocksRows16Tab2d;
            return form_code(kFormBlk, r16 ? 16 : 8, true, stride_t, in.tab_vmode ? kFormTabRowvec : r16 ? kFormTab2d16 : kFormTab2d, in.label_free);
        }
        return form_code(kFormK32, 8, true, 0, lut);
    case kEntryFusedBin: {
        const int rows = in.tab_vmode ? (in.blocks8 > kBlocksRows16 ? 16 : 8) : (in.stride == 3 && in.blocks8 <= kBlocksBinRows4 ? 4 : 8);
        return form_code(kFormBin, rows, true, stride_t, subsampled);
    }
    case kEntryPre: return in.blk_applies ? form_code(kFormPre, 8, true, stride_t, subsampled) : kFormNone;
    case kEntryGenericFull: return form_code(kFormGeneric, 0, false, 0, kFormTabNone);
    case kEntryGenericFused: return form_code(kFormGeneric, 0, true, 0, kFormTabNone);
    default: return form_code(kFormGenericRec, 0, true, 0, kFormTabNone);
    }
}

// A table of forms is an array of rows with a member `code`: its codes into `codes` (at most `cap`), returns how many there are
template <class Row, size_t N> int row_codes(const Row (&rows)[N], uint32_t* codes, int cap) {
    for (int i = 0; i < (int)N && i < cap; i++) codes[i] = rows[i].code;
    return (int)N;
}
// The row of `code`, nullptr where the table has none
template <class Row, size_t N> constexpr const Row* find_row(const Row (&rows)[N], uint32_t code) {
    for (size_t i = 0; i < N; i++)
        if (rows[i].code == code) return &rows[i];
    return nullptr;
}

// Adds `code` to the process-wide set (thread-safe).  Called where a launch is enqueued or recorded into a graph; a replay adds nothing.
void note_form(uint32_t code);
// The set so far, at most `cap` codes into `codes`; returns how many there are (-2: more than the record holds).  clear: empty it.
int forms_seen(uint32_t* codes, int cap, bool clear);
// Every code a launch function can note: the codes of the tables' rows (assign.hip, preempt.hip), as row_codes
int assign_forms(uint32_t* codes, int cap);
int preempt_forms(uint32_t* codes, int cap);

}  // namespace fslic
