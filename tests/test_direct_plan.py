"""The kernel choice of the direct path (vgx_choose_direct in vgx_direct_run.hip) as a table: shape and options in, plan or refusal
out.  The choice is a pure function of about 25 integers, reached through ``vgx_test_direct_plan``: no device, no engine.

The expected column records what the dispatch did when it was still part of ``direct_core`` (it was generated from that code, not
from the function under test), so a row changes only with a deliberate change of behaviour.  Three groups of rows pin behaviour that
ADVICE.md questions (items 2, 3 and 5): each carries a comment naming the item, and the fix of an item flips exactly those rows."""
import pytest

from vgsim_amd import _capi

WAVE, LANES, QUAD, QUADG, SOLO, LONE, QUADF = 1, 2, 3, 4, 5, 6, 7

PLAN_FIELDS = [name for name, _ in _capi.VgxDirectPlan._fields_]


def plan(kernel, **fields):
    """A full vgx_direct_plan: what is not named is 0 (exact mode, PCG64 stream, no field of a kernel that was not chosen)."""
    out = dict.fromkeys(PLAN_FIELDS, 0)
    out.update(fields, kernel=kernel)
    return out


def model(**fields):
    """A shape that came through vgx_set_state (fresh_state), with population sizes far below every threshold; what is not named is 0."""
    out = dict(start_max_nocc=1, max_size=1000000, hosts_below_2p53=1, fresh_state=1, suscep_cumul0_zero=1)
    out.update(fields)
    return out


# a small model with several groups and classes (the Table-3 kind): both latency kernels and the general row kernel take it
SMALL = model(P=10, sites=2, H=16, S=3, C=4, CB=2, cap=16, n_seg=4, n_solo_seg=4, solo_npass0=2, solo_npass1=2, solo_ncls=2,
              solo_maxnnz=2, start_lone_rows=10)
# the same with 256 haplotypes: too many for the dense latency kernel (vgx_solo.hip)
MID = dict(SMALL, sites=4, H=256, cap=256)
# ... and 100 populations: beyond the 64 of the list latency kernel (vgx_lone.hip) and the one register slot of the general row kernel
WIDE = dict(MID, P=100, start_lone_rows=100)
# one rate class, one group, two populations, four haplotypes
ONE = model(P=2, sites=1, H=4, S=1, C=1, CB=1, cap=4, n_seg=1, n_solo_seg=1, solo_npass0=1, solo_npass1=1, solo_ncls=1,
            solo_maxnnz=1, start_lone_rows=2, have_counts32=1, tot_sus_is_sus=1)
# ... with one haplotype: P * H * S = 2
TINY = dict(ONE, sites=0, H=1, cap=1)
# one class, eight populations, 2^26 haplotypes in lists of 2^24 entries; the one-class heap of vgx_lone.hip has 600 rows at 160 KB of LDS
# (up to 256 replicates) and 290 at 80 KB
BIG = dict(ONE, P=8, sites=13, H=1 << 26, cap=1 << 24, start_lone_rows=8)

# (name, model, what the row changes in it, opts.mode, opts.kernel, the plan or the refusal)
CASES = [
    # ---- every kernel as the automatic choice ----
    ('lanes_from_131072_replicates_of_a_minimal_model', TINY, dict(R=131072), 0, 0,
     plan(LANES)),
    ('no_lanes_below_131072', TINY, dict(R=131071), 0, 0,
     plan(QUAD)),
    ('no_lanes_beyond_P_H_S_4', ONE, dict(R=131072), 0, 0,
     plan(QUAD)),
    ('solo_below_8192_replicates_of_a_one_class_model', ONE, dict(R=8191), 0, 0,
     plan(SOLO, solo_mig_in_lds=1, solo_compact=1)),
    ('quad_from_8192_replicates_of_a_one_class_model', ONE, dict(R=8192), 0, 0,
     plan(QUAD)),
    ('quad_long_lists_beyond_one_tile', BIG, dict(R=8192, start_max_nocc=65), 0, 0,
     plan(QUAD, long_lists=1, leaves32=1)),
    ('quad_one_tile', BIG, dict(R=8192, start_max_nocc=64), 0, 0,
     plan(QUAD)),
    ('solo_single_trajectory_of_a_small_general_model', SMALL, dict(R=1), 0, 0,
     plan(SOLO, solo_mig_in_lds=1, solo_compact=2)),
    ('solo_compact_and_small_at_any_ensemble_size', SMALL, dict(R=16384), 0, 0,
     plan(SOLO, solo_mig_in_lds=1, solo_compact=2)),
    ('solo_general_layout_only_below_2048', SMALL, dict(R=2047, solo_ncls=5), 0, 0,
     plan(SOLO, solo_mig_in_lds=1)),
    ('solo_general_layout_not_from_2048', SMALL, dict(R=2048, solo_ncls=5), 0, 0,
     plan(QUADG)),
    ('solo_compact_layout_switched_off_by_VGX_SOLO_GENERAL', SMALL, dict(R=1, solo_general=1), 0, 0,
     plan(SOLO, solo_mig_in_lds=1)),
    ('lone_fresh_state_1536_replicates_half_the_heap_free', BIG, dict(R=1536, start_lone_rows=145), 0, 0,
     plan(LONE, lone_lds_bytes=81920, fallback_kernel=QUAD)),
    ('lone_not_when_more_than_half_the_heap_is_taken', BIG, dict(R=1536, start_lone_rows=146), 0, 0,
     plan(QUAD)),
    ('lone_one_trajectory_160KB_heap', BIG, dict(R=1, start_lone_rows=300), 0, 0,
     plan(LONE, lone_lds_bytes=163840, fallback_kernel=QUAD)),
    ('lone_not_from_1537_replicates', BIG, dict(R=1537), 0, 0,
     plan(QUAD)),
    ('lone_not_on_a_continued_state', BIG, dict(R=1, fresh_state=0), 0, 0,
     plan(QUAD)),
    ('lone_not_with_VGX_NO_LONE', BIG, dict(R=1, no_lone=1), 0, 0,
     plan(QUAD)),
    ('lone_general_form', MID, dict(R=1), 0, 0,
     plan(LONE, lone_general=1, lone_lds_bytes=163840, fallback_kernel=QUAD)),
    ('quadg_from_2048_replicates', MID, dict(R=2048), 0, 0,
     plan(QUADG)),
    ('quadg_from_2048_replicates_at_100_populations', WIDE, dict(R=2048), 0, 0,
     plan(QUADG)),
    ('quadg_few_replicates_P16_several_groups', MID, dict(R=16, P=16, fresh_state=0), 0, 0,
     plan(QUADG)),
    ('quadg_few_replicates_P16_several_classes', MID, dict(R=16, P=16, S=1, C=2, fresh_state=0), 0, 0,
     plan(QUADG)),
    ('quadg_few_replicates_P16_lockdown', MID, dict(R=16, P=16, S=1, C=1, CB=1, ld_possible=1, fresh_state=0), 0, 0,
     plan(QUADG)),
    ('wave_few_replicates_P16_one_class_no_lockdown', MID, dict(R=16, P=16, S=1, C=1, CB=1, fresh_state=0), 0, 0,
     plan(WAVE)),
    ('wave_few_replicates_P17', MID, dict(R=16, P=17, fresh_state=0), 0, 0,
     plan(WAVE)),
    ('wave_few_replicates_100_populations', WIDE, dict(R=2047), 0, 0,
     plan(WAVE)),
    ('wave_nine_groups_at_any_ensemble_size', WIDE, dict(R=16384, S=9), 0, 0,
     plan(WAVE)),
    ('quadf_fast_one_class', ONE, dict(R=16384), 1, 0,
     plan(QUADF, mode=1, fast=1, leaves32=1)),
    ('quadf_fast_one_class_single_trajectory', ONE, dict(R=1), 1, 0,
     plan(QUADF, mode=1, fast=1, leaves32=1)),
    # ---- every refusal message ----
    ('refused_recombination_in_fast_mode', SMALL, dict(R=1, recomb=1), 1, 0,
     'vgx_simulate_direct: recombination runs in exact mode only'),
    ('refused_kernel_7', SMALL, dict(R=1), 0, 7,
     'vgx_simulate_direct: kernel must be 0..6'),
    ('refused_kernel_minus_1', SMALL, dict(R=1), 0, -1,
     'vgx_simulate_direct: kernel must be 0..6'),
    ('refused_lanes_17_populations', SMALL, dict(R=1, P=17), 0, 2,
     'vgx_simulate_direct: the lane-per-replicate kernel needs exact mode, popNum <= 16, popNum * hapNum <= 1024 and susNum <= 8'),
    ('refused_lanes_in_fast_mode', TINY, dict(R=1), 1, 2,
     'vgx_simulate_direct: the lane-per-replicate kernel needs exact mode, popNum <= 16, popNum * hapNum <= 1024 and susNum <= 8'),
    ('refused_solo_256_haplotypes', MID, dict(R=1), 0, 5,
     'vgx_simulate_direct: the single-trajectory kernel needs exact mode, hapNum <= 64, popNum <= 128, susNum <= 16 and a model that fits 160 KB of LDS'),
    ('refused_lone_65_populations', MID, dict(R=1, P=65), 0, 6,
     'vgx_simulate_direct: the single-trajectory kernel for large haplotype spaces needs exact mode, popNum <= 64, susNum <= 16, at most 64 rate classes and 16 transmission/susceptibility classes, hapNum <= 2^26, no recombination'),
    ('refused_row_kernels_nine_groups', MID, dict(R=1, S=9), 0, 3,
     'vgx_simulate_direct: the four-replicates-per-wavefront kernels need popNum <= 128, susNum <= 8, at most 64 rate classes and 16 transmission/susceptibility classes'),
    ('refused_quadg_65_segments', MID, dict(R=1, n_seg=65), 0, 4,
     'vgx_simulate_direct: the general four-replicates-per-wavefront kernel needs exact mode, popNum <= 128, susNum <= 8, at most 64 rate classes and 16 transmission/susceptibility classes'),
    ('refused_checks_run_in_order_kernel_range_after_recombination', SMALL, dict(R=1, recomb=1), 2, 9,
     'vgx_simulate_direct: recombination runs in exact mode only'),
    # ---- kernels that were asked for ----
    ('asked_wave', ONE, dict(R=16384), 0, 1,
     plan(WAVE)),
    ('asked_lanes', SMALL, dict(R=16), 0, 2,
     plan(LANES)),
    ('asked_row_kernel_one_class', ONE, dict(R=16), 0, 3,
     plan(QUAD)),
    ('asked_row_kernel_general', SMALL, dict(R=16), 0, 3,
     plan(QUADG)),
    ('asked_row_kernel_fast_one_class', ONE, dict(R=16), 1, 3,
     plan(QUADF, mode=1, fast=1, leaves32=1)),
    ('asked_quadg_on_a_one_class_model', ONE, dict(R=16), 0, 4,
     plan(QUADG)),
    ('asked_solo_16384_replicates', ONE, dict(R=16384), 0, 5,
     plan(SOLO, solo_mig_in_lds=1, solo_compact=1)),
    ('asked_lone_continued_state_no_fallback', BIG, dict(R=4096, fresh_state=0), 0, 6,
     plan(LONE, lone_lds_bytes=81920)),
    ('asked_wave_fast', SMALL, dict(R=16), 1, 1,
     plan(WAVE, mode=1, fast=1)),
    # ---- the mode remapped ----
    ('fast_on_a_general_model_served_exactly', MID, dict(R=16384), 1, 0,
     plan(QUADG)),
    ('fast_on_a_small_general_model_served_by_solo', SMALL, dict(R=16384), 1, 0,
     plan(SOLO, solo_mig_in_lds=1, solo_compact=2)),
    ('fast_general_below_2048_P_above_16_back_on_the_wave_kernels_fast_form', WIDE, dict(R=2047), 1, 0,
     plan(WAVE, mode=1, fast=1)),
    ('fast_with_a_kernel_asked_for_is_not_remapped', MID, dict(R=16384), 1, 4,
     'vgx_simulate_direct: the general four-replicates-per-wavefront kernel needs exact mode, popNum <= 128, susNum <= 8, at most 64 rate classes and 16 transmission/susceptibility classes'),
    ('philox_on_quadg', MID, dict(R=16384), 2, 0,
     plan(QUADG, philox=1)),
    ('philox_on_solo', SMALL, dict(R=1), 2, 0,
     plan(SOLO, philox=1, solo_mig_in_lds=1, solo_compact=2)),
    ('philox_on_lone', MID, dict(R=1), 2, 0,
     plan(LONE, philox=1, lone_general=1, lone_lds_bytes=163840, fallback_kernel=QUAD, fallback_mode=2)),
    # kernel=5 takes mode=2 (remapped), though its refusal says 'needs exact mode'
    ('philox_asked_solo', SMALL, dict(R=1), 2, 5,
     plan(SOLO, philox=1, solo_mig_in_lds=1, solo_compact=2)),
    # kernel=6 takes mode=2 (remapped), though its refusal says 'needs exact mode'
    ('philox_asked_lone', MID, dict(R=1), 2, 6,
     plan(LONE, philox=1, lone_general=1, lone_lds_bytes=163840)),
    ('philox_asked_row_kernel_general', MID, dict(R=16), 2, 3,
     plan(QUADG, philox=1)),
    ('philox_asked_row_kernel_one_class', BIG, dict(R=16), 2, 3,
     plan(QUADF, mode=2, fast=1, philox=1, leaves32=1)),
    ('philox_asked_quadg_general', MID, dict(R=16), 2, 4,
     plan(QUADG, philox=1)),
    # kernel=4 with mode=2 on a one-class model is refused with 'needs exact mode', though the general row kernel serves mode=2 for general models
    ('philox_asked_quadg_one_class_refused', ONE, dict(R=16), 2, 4,
     'vgx_simulate_direct: the general four-replicates-per-wavefront kernel needs exact mode, popNum <= 128, susNum <= 8, at most 64 rate classes and 16 transmission/susceptibility classes'),
    # lands on solo (the R < 8192 bound of one-class models is skipped under the remap); the fix puts it on QUADF, mode 2, fast 1
    ('philox_one_class_100000_replicates', ONE, dict(R=100000), 2, 0,
     plan(SOLO, philox=1, solo_mig_in_lds=1, solo_compact=1)),
    ('philox_one_class_large_haplotype_space_on_quadf', BIG, dict(R=8192), 2, 0,
     plan(QUADF, mode=2, fast=1, philox=1, leaves32=1)),
    ('philox_general_below_2048_P_above_16_back_in_mode_2', WIDE, dict(R=2047), 2, 0,
     plan(WAVE, mode=2, fast=1, philox=1)),
    ('philox_asked_wave', SMALL, dict(R=16), 2, 1,
     plan(WAVE, mode=2, fast=1, philox=1)),
    # ---- the fallback of a full lone heap ----
    ('fallback_one_class_to_the_row_kernel', BIG, dict(R=1), 0, 0,
     plan(LONE, lone_lds_bytes=163840, fallback_kernel=QUAD)),
    ('fallback_general_to_the_row_kernel', MID, dict(R=1), 0, 0,
     plan(LONE, lone_general=1, lone_lds_bytes=163840, fallback_kernel=QUAD)),
    ('fallback_nine_groups_to_the_wave_kernel', MID, dict(R=1, S=9), 0, 0,
     plan(LONE, lone_general=1, lone_lds_bytes=163840, fallback_kernel=WAVE)),
    ('fallback_philox_nine_groups_to_the_wave_kernel_in_mode_2', MID, dict(R=1, S=9), 2, 0,
     plan(LONE, philox=1, lone_general=1, lone_lds_bytes=163840, fallback_kernel=WAVE, fallback_mode=2)),
    ('fallback_fast_request_repeats_in_mode_0', MID, dict(R=1), 1, 0,
     plan(LONE, lone_general=1, lone_lds_bytes=163840, fallback_kernel=QUAD)),
    # the fallback kernel 3 comes from predicates seen under the remapped mode 0, the fallback mode is 2 ...
    ('fallback_philox_one_class_not_quad_shape', BIG, dict(R=1, suscep_cumul0_zero=0), 2, 0,
     plan(LONE, philox=1, lone_general=1, lone_lds_bytes=163840, fallback_kernel=QUAD, fallback_mode=2)),
    # ... and that request is refused; the fix makes the fallback one that this row accepts (the wavefront kernel)
    ('fallback_philox_one_class_not_quad_shape_second_pass', BIG, dict(R=1, suscep_cumul0_zero=0), 2, 3,
     'vgx_simulate_direct: the four-replicates-per-wavefront kernels need popNum <= 128, susNum <= 8, at most 64 rate classes and 16 transmission/susceptibility classes'),
    # ---- recombination ----
    ('recomb_single_trajectory_on_solo', SMALL, dict(R=1, recomb=1), 0, 0,
     plan(SOLO, solo_mig_in_lds=1, solo_compact=2)),
    ('recomb_one_class_is_no_row_kernel_shape', ONE, dict(R=16384, recomb=1), 0, 0,
     plan(SOLO, solo_mig_in_lds=1, solo_compact=1)),
    ('recomb_ensemble_on_quadg', MID, dict(R=16384, recomb=1), 0, 0,
     plan(QUADG)),
    ('recomb_never_on_lone', MID, dict(R=1, recomb=1), 0, 0,
     plan(QUADG)),
    ('recomb_lone_refused', MID, dict(R=1, recomb=1), 0, 6,
     'vgx_simulate_direct: the single-trajectory kernel for large haplotype spaces needs exact mode, popNum <= 64, susNum <= 16, at most 64 rate classes and 16 transmission/susceptibility classes, hapNum <= 2^26, no recombination'),
    ('recomb_few_replicates_100_populations_on_wave', WIDE, dict(R=16, recomb=1), 0, 0,
     plan(WAVE)),
    ('recomb_lanes_only_when_asked_for', TINY, dict(R=131072, recomb=1), 0, 0,
     plan(SOLO, solo_mig_in_lds=1, solo_compact=1)),
    ('recomb_asked_lanes', MID, dict(R=16, recomb=1), 0, 2,
     plan(LANES)),
    ('recomb_asked_lanes_dense_arrays_beyond_2p24', BIG, dict(R=16, recomb=1), 0, 2,
     'vgx_simulate_direct: the lane-per-replicate kernel needs exact mode, popNum <= 16, popNum * hapNum <= 1024 and susNum <= 8'),
    ('recomb_philox_refused', SMALL, dict(R=1, recomb=1), 2, 0,
     'vgx_simulate_direct: recombination runs in exact mode only'),
    # ---- thresholds ----
    ('size_2p31_minus_1_on_quad', ONE, dict(R=8192, max_size=(1 << 31) - 1), 0, 0,
     plan(QUAD)),
    ('size_2p31_off_quad', ONE, dict(R=8192, max_size=1 << 31), 0, 0,
     plan(SOLO, solo_mig_in_lds=1, solo_compact=1)),
    ('size_2p31_off_lone', MID, dict(R=1, max_size=1 << 31), 0, 0,
     plan(QUADG)),
    ('size_2p52_minus_1_on_solo', ONE, dict(R=1, max_size=(1 << 52) - 1), 0, 0,
     plan(SOLO, solo_mig_in_lds=1, solo_compact=1)),
    ('size_2p52_off_solo', ONE, dict(R=1, max_size=1 << 52), 0, 0,
     plan(WAVE)),
    ('size_2p52_solo_refused', ONE, dict(R=1, max_size=1 << 52), 0, 5,
     'vgx_simulate_direct: the single-trajectory kernel needs exact mode, hapNum <= 64, popNum <= 128, susNum <= 16 and a model that fits 160 KB of LDS'),
    ('hosts_2p53_off_quad', ONE, dict(R=8192, max_size=1 << 53, hosts_below_2p53=0), 0, 0,
     plan(QUADG)),
    ('cap_2p24_on_quad', BIG, dict(R=8192, cap=1 << 24), 0, 0,
     plan(QUAD)),
    ('cap_above_2p24_off_quad', BIG, dict(R=8192, cap=(1 << 24) + 64), 0, 0,
     plan(QUADG)),
    ('immunity_loss_from_group_0_off_quad', ONE, dict(R=8192, suscep_cumul0_zero=0), 0, 0,
     plan(SOLO, solo_mig_in_lds=1, solo_compact=1)),
    ('susceptible_totals_differ_off_quad', ONE, dict(R=8192, tot_sus_is_sus=0), 0, 0,
     plan(SOLO, solo_mig_in_lds=1, solo_compact=1)),
    ('lockdown_off_quad', ONE, dict(R=8192, ld_possible=1), 0, 0,
     plan(SOLO, solo_mig_in_lds=1, solo_compact=1)),
    ('solo_migration_rates_in_hbm', SMALL, dict(R=1, P=128, H=16, S=1, C=1, CB=1, solo_maxnnz=1), 0, 0,
     plan(SOLO)),
]


def test_names_are_unique():
    names = [c[0] for c in CASES]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("name,base,change,mode,kernel,expected", CASES, ids=[c[0] for c in CASES])
def test_direct_plan(name, base, change, mode, kernel, expected):
    shape = dict(base, **change)
    if isinstance(expected, str):
        with pytest.raises(_capi.VgxError) as err:
            _capi.direct_plan(shape, mode=mode, kernel=kernel)
        assert err.value.code == 1                       # VGX_ERR_ARG
        assert str(err.value) == "libvgx error 1: " + expected
    else:
        assert _capi.direct_plan(shape, mode=mode, kernel=kernel) == expected


def test_every_kernel_is_an_automatic_choice_and_every_refusal_occurs():
    auto = {c[5]["kernel"] for c in CASES if c[4] == 0 and not isinstance(c[5], str)}
    assert auto == {WAVE, LANES, QUAD, QUADG, SOLO, LONE, QUADF}
    assert len({c[5] for c in CASES if isinstance(c[5], str)}) == 7
