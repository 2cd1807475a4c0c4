"""ctypes binding of libvgx.so (C ABI in ``include/vgx.h``): the only way the Python host layer reaches
the HIP kernels.  There is no CPU fallback: a missing library or a missing GPU raises ``RuntimeError``.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VGX_LIBRARY", os.path.join(HERE, "libvgx.so"))  # VGX_LIBRARY: diagnostic builds only

_F = C.POINTER(C.c_double)
_I = C.POINTER(C.c_int64)

VGX_OK = 0


class VgxDims(C.Structure):
    _fields_ = [("sites", C.c_int64), ("hapNum", C.c_int64), ("popNum", C.c_int64), ("susNum", C.c_int64)]


class VgxParams(C.Structure):
    _fields_ = [("bRate", _F), ("dRate", _F), ("sRate", _F), ("mRate", _F), ("hapMutType", _F),
                ("susceptibility", _F), ("suscType", _I), ("suscepTransition", _F), ("sizes", _I),
                ("contactDensityBeforeLockdown", _F), ("contactDensityAfterLockdown", _F), ("startLD", _F),
                ("endLD", _F), ("samplingMultiplier", _F), ("migrationRates", _F)]


class VgxState(C.Structure):
    _fields_ = [("susceptible", _I), ("infectious", _I), ("initial_susceptible", _I), ("initial_infectious", _I),
                ("totalSusceptible", _I), ("totalInfectious", _I), ("lockdownON", _I), ("contactDensity", _F),
                ("first_simulation", C.c_int64), ("globalInfectious", C.c_int64),
                ("bCounter", C.c_int64), ("dCounter", C.c_int64), ("sCounter", C.c_int64), ("mCounter", C.c_int64),
                ("iCounter", C.c_int64), ("swapLockdown", C.c_int64), ("migPlus", C.c_int64), ("migNonPlus", C.c_int64),
                ("good_attempt", C.c_int64),
                ("currentTime", C.c_double), ("totalRate", C.c_double), ("totalMigrationRate", C.c_double),
                ("tau_l", C.c_double), ("ev_ptr", C.c_int64), ("ev_size", C.c_int64)]


class VgxRunOpts(C.Structure):
    _fields_ = [("record_events", C.c_int64), ("max_loop_factor", C.c_int64), ("traj_points", C.c_int64),
                ("traj_t0", C.c_double), ("traj_t1", C.c_double), ("mode", C.c_int64), ("kernel", C.c_int64),
                ("reserved", C.c_int64 * 2)]


class VgxCounters(C.Structure):
    _fields_ = [("ev_ptr", C.c_int64), ("ev_first_new", C.c_int64), ("loop_iterations", C.c_int64),
                ("restarts", C.c_int64), ("lockdown_records", C.c_int64), ("error", C.c_int64),
                ("multievent_rows", C.c_int64), ("reserved", C.c_int64 * 5)]


class VgxGenealogyIO(C.Structure):
    _fields_ = [("popNum", C.c_int64), ("hapNum", C.c_int64), ("sCounter", C.c_int64), ("ev_ptr", C.c_int64),
                ("ev_times", _F), ("ev_types", _I), ("ev_haplotypes", _I), ("ev_populations", _I),
                ("ev_newHaplotypes", _I), ("ev_newPopulations", _I),
                ("mev_rows", C.c_int64), ("mev_num", _I), ("mev_times", _F), ("mev_types", _I), ("mev_haplotypes", _I),
                ("mev_populations", _I), ("mev_newHaplotypes", _I), ("mev_newPopulations", _I),
                ("infectious", _I), ("rng_state", C.c_uint64 * 4), ("rng_has_uint32", C.c_int64), ("rng_uinteger", C.c_uint64),
                ("tree", _I), ("tree_pop", _I), ("times", _F),
                ("mut_cap", C.c_int64), ("mut_n", C.c_int64), ("mut_node", _I), ("mut_AS", _I), ("mut_DS", _I),
                ("mut_site", _I), ("mut_time", _F),
                ("mig_cap", C.c_int64), ("mig_n", C.c_int64), ("mig_node", _I), ("mig_old", _I), ("mig_new", _I),
                ("mig_time", _F), ("nodes_used", C.c_int64)]


class VgxGenealogiesIO(C.Structure):
    _fields_ = [("n", C.c_int64), ("replicates", _I), ("rng_state", C.POINTER(C.c_uint64)),
                ("node_off", _I), ("mut_off", _I), ("mig_off", _I),
                ("tree", _I), ("tree_pop", _I), ("times", _F),
                ("mut_node", _I), ("mut_AS", _I), ("mut_DS", _I), ("mut_site", _I), ("mut_time", _F),
                ("mig_node", _I), ("mig_old", _I), ("mig_new", _I), ("mig_time", _F),
                ("status", _I), ("status_arg", _I), ("nodes_used", _I), ("mut_n", _I), ("mig_n", _I),
                ("rng_out", C.POINTER(C.c_uint64)), ("layout", C.c_int64), ("passes", C.c_int64), ("ms", C.c_double * 3)]


class VgxTauGenealogyPrefix(C.Structure):
    _fields_ = [("ev_ptr", C.c_int64), ("ev_times", _F), ("ev_types", _I), ("ev_haplotypes", _I), ("ev_populations", _I),
                ("ev_newHaplotypes", _I), ("ev_newPopulations", _I),
                ("mev_rows", C.c_int64), ("mev_num", _I), ("mev_times", _F), ("mev_types", _I), ("mev_haplotypes", _I),
                ("mev_populations", _I), ("mev_newHaplotypes", _I), ("mev_newPopulations", _I)]


class VgxTauGenealogiesIO(C.Structure):
    _fields_ = [("n", C.c_int64), ("replicates", _I), ("rng_state", C.POINTER(C.c_uint64)),
                ("node_off", _I), ("mut_off", _I), ("mig_off", _I),
                ("tree", _I), ("tree_pop", _I), ("times", _F),
                ("mut_node", _I), ("mut_AS", _I), ("mut_DS", _I), ("mut_site", _I), ("mut_time", _F),
                ("mig_node", _I), ("mig_old", _I), ("mig_new", _I), ("mig_time", _F),
                ("status", _I), ("status_arg", _I), ("nodes_used", _I), ("mut_n", _I), ("mig_n", _I),
                ("rng_out", C.POINTER(C.c_uint64)), ("passes", C.c_int64), ("ms", C.c_double * 3)]


TAU_STEP_ROWS_MAX = 8192   # raw multievent rows of one step the device pass sorts (vgx.h: the step bound)
GW_STEP_ROWS = 10          # the status of a replicate with a longer step


class VgxTimelinesIO(C.Structure):
    _fields_ = [("n", C.c_int64), ("replicates", _I), ("step_num", C.c_int64), ("semantics", C.c_int64),
                ("n_inf", C.c_int64), ("inf_pop", _I), ("inf_hap", _I), ("n_sus", C.c_int64), ("sus_pop", _I), ("sus_grp", _I),
                ("time_points", _F), ("inf_data", _F), ("inf_sample", _F), ("sus_data", _F), ("last_point", _I),
                ("loc_cap", C.c_int64), ("loc_n", _I), ("loc_state", _I), ("loc_pop", _I), ("loc_time", _F),
                ("passes", C.c_int64), ("ms", C.c_double * 3)]


class VgxTimelinesChain(C.Structure):
    _fields_ = [("popNum", C.c_int64), ("hapNum", C.c_int64), ("susNum", C.c_int64), ("ev_ptr", C.c_int64),
                ("ev_times", _F), ("ev_types", _I), ("ev_haplotypes", _I), ("ev_populations", _I),
                ("ev_newHaplotypes", _I), ("ev_newPopulations", _I),
                ("currentTime", C.c_double), ("step_num", C.c_int64), ("semantics", C.c_int64),
                ("n_inf", C.c_int64), ("inf_pop", _I), ("inf_hap", _I), ("inf_start", _I),
                ("n_sus", C.c_int64), ("sus_pop", _I), ("sus_grp", _I), ("sus_start", _I),
                ("time_points", _F), ("inf_data", _F), ("inf_sample", _F), ("sus_data", _F), ("last_point", C.c_int64)]


class VgxTimelinesPrefix(C.Structure):
    _fields_ = [("ev_ptr", C.c_int64), ("ev_times", _F), ("ev_types", _I), ("ev_haplotypes", _I), ("ev_populations", _I),
                ("ev_newHaplotypes", _I), ("ev_newPopulations", _I),
                ("mev_rows", C.c_int64), ("mev_num", _I), ("mev_types", _I), ("mev_haplotypes", _I), ("mev_populations", _I),
                ("mev_newHaplotypes", _I), ("mev_newPopulations", _I),
                ("loc_n", C.c_int64), ("loc_state", _I), ("loc_pop", _I), ("loc_time", _F)]


class VgxTauTimelinesChain(C.Structure):
    _fields_ = [("chain", VgxTimelinesChain), ("mev_rows", C.c_int64), ("mev_num", _I), ("mev_types", _I), ("mev_haplotypes", _I),
                ("mev_populations", _I), ("mev_newHaplotypes", _I), ("mev_newPopulations", _I)]


class VgxTrajSummaryIO(C.Structure):
    _fields_ = [("G", C.c_int64), ("group_of", _I), ("K", C.c_int64), ("ranks", _I), ("count", _I), ("sum", _I),
                ("sumsq", C.POINTER(C.c_uint64)), ("min", _I), ("max", _I), ("stat", _I), ("passes", C.c_int64), ("ms", C.c_double * 3)]


class VgxIncidenceIO(C.Structure):
    _fields_ = [("n", C.c_int64), ("replicates", _I), ("T", C.c_int64), ("edges", _F), ("hap_mask", C.POINTER(C.c_uint32)),
                ("counts", C.POINTER(C.c_int32)), ("outside", _I), ("summary", C.POINTER(VgxTrajSummaryIO)),
                ("passes", C.c_int64), ("ms", C.c_double * 3)]


class VgxPrevalenceIO(C.Structure):
    _fields_ = [("n", C.c_int64), ("replicates", _I), ("T", C.c_int64), ("grid", _F), ("V", C.c_int64), ("variant_of", C.POINTER(C.c_int32)),
                ("values", C.POINTER(C.c_int32)), ("final", C.POINTER(C.c_int32)), ("outside", _I), ("summary", C.POINTER(VgxTrajSummaryIO)),
                ("passes", C.c_int64), ("ms", C.c_double * 3)]


class VgxLineagesIO(C.Structure):
    _fields_ = [("n", C.c_int64), ("replicates", _I), ("rng_state", C.POINTER(C.c_uint64)), ("T", C.c_int64), ("grid", _F),
                ("V", C.c_int64), ("variant_of", C.POINTER(C.c_int32)), ("values", C.POINTER(C.c_int32)), ("root", C.POINTER(C.c_int32)),
                ("status", _I), ("status_arg", _I), ("records", _I), ("rng_out", C.POINTER(C.c_uint64)),
                ("summary", C.POINTER(VgxTrajSummaryIO)), ("passes", C.c_int64), ("ms", C.c_double * 3), ("kernel_ms", C.c_double * 3)]


class VgxTauLineagesIO(C.Structure):   # VgxLineagesIO with six generator words per walk and four kernel stages
    _fields_ = VgxLineagesIO._fields_[:-1] + [("kernel_ms", C.c_double * 4)]


class VgxTreeEventsIO(C.Structure):   # VgxLineagesIO with `counts` for `values`, no root and two kernel stages
    _fields_ = ([("counts", t) if f == "values" else (f, t) for f, t in VgxLineagesIO._fields_[:-1] if f != "root"]
                + [("kernel_ms", C.c_double * 2)])


class VgxTauTreeEventsIO(C.Structure):   # VgxTreeEventsIO with six generator words per walk and three kernel stages
    _fields_ = VgxTreeEventsIO._fields_[:-1] + [("kernel_ms", C.c_double * 3)]


TREE_EVENT_CHANNELS = ("samples", "coalescences", "mutations_within", "mutations_out", "mutations_in", "departures", "arrivals")


class VgxTreeShapesIO(C.Structure):
    _fields_ = [("n", C.c_int64), ("replicates", _I), ("rng_state", C.POINTER(C.c_uint64)), ("stats", _I), ("lengths", _F),
                ("status", _I), ("status_arg", _I), ("rng_out", C.POINTER(C.c_uint64)), ("passes", C.c_int64), ("ms", C.c_double * 4)]


class VgxTauTreeShapesIO(C.Structure):   # VgxTreeShapesIO with six generator words per walk, three times and four kernel stages
    _fields_ = VgxTreeShapesIO._fields_[:-1] + [("ms", C.c_double * 3), ("kernel_ms", C.c_double * 4)]


# the columns of vgx_tree_shapes_io.stats and .lengths (vgx_tree_shape.h)
TREE_SHAPE_STATS = ("tips", "internal", "cherries", "pitchforks", "sackin", "colless", "max_depth", "depth_sumsq", "ladder_nodes", "max_ladder",
                    "root_event", "last_tip_event")
TREE_SHAPE_LENGTHS = ("root_time", "last_tip_time", "length", "external_length", "length_sumsq", "tip_height_sum", "max_branch")
GW_BAD_TREE = 13   # the status of a replicate whose tree breaks the structure the shape sweep needs (status_arg: the node)


class VgxMutationSpectrumIO(C.Structure):
    _fields_ = [("n", C.c_int64), ("replicates", _I), ("rng_state", C.POINTER(C.c_uint64)), ("spectrum", _I), ("substitutions", _I),
                ("sums", _I), ("stats", _I), ("status", _I), ("status_arg", _I), ("rng_out", C.POINTER(C.c_uint64)), ("sites", C.c_int64),
                ("passes", C.c_int64), ("ms", C.c_double * 3)]


class VgxTauMutationSpectrumIO(C.Structure):   # VgxMutationSpectrumIO with six generator words per walk and three kernel stages
    _fields_ = VgxMutationSpectrumIO._fields_ + [("kernel_ms", C.c_double * 3)]


# the columns of vgx_mutation_spectrum_io.sums and .stats (vgx_mutation_spectrum.h)
MUTATION_SPECTRUM_BINS = 32
MUTATION_SPECTRUM_SUMS = ("clade_sum", "clade_sumsq", "pair_sum")
MUTATION_SPECTRUM_STATS = ("tips", "mutations", "fixed", "max_clade")
GW_BAD_RECORD = 14   # the status of a replicate with a mutation record outside its tree or the model (status_arg: the record)


class VgxIntroductionsIO(C.Structure):
    _fields_ = [("n", C.c_int64), ("replicates", _I), ("rng_state", C.POINTER(C.c_uint64)), ("tips_by_pop", _I), ("imports", _I), ("into", _I),
                ("spectrum", _I), ("stats", _I), ("status", _I), ("status_arg", _I), ("rng_out", C.POINTER(C.c_uint64)), ("pops", C.c_int64),
                ("passes", C.c_int64), ("ms", C.c_double * 3)]


class VgxTauIntroductionsIO(C.Structure):   # VgxIntroductionsIO with six generator words per walk and three kernel stages
    _fields_ = VgxIntroductionsIO._fields_ + [("kernel_ms", C.c_double * 3)]


# the columns of vgx_introductions_io.into and .stats (vgx_introductions.h)
INTRODUCTIONS_BINS = 32
INTRODUCTIONS_INTO = ("count", "clade_sum", "local_sum", "local_sumsq", "empty", "max_local")
INTRODUCTIONS_STATS = ("tips", "introductions", "root_pop", "root_local", "max_local", "max_clade", "empty", "pops_with_tips")
INTRODUCTIONS_POPS_MAX = 1024
GW_BAD_LABEL = 15   # the status of a replicate with a node label outside the model (status_arg: the node)


class VgxFlowsIO(C.Structure):
    _fields_ = [("n", C.c_int64), ("replicates", _I), ("T", C.c_int64), ("edges", _F), ("V", C.c_int64), ("variant_of", C.POINTER(C.c_int32)),
                ("within", C.c_int32), ("counts", C.POINTER(C.c_int32)), ("outside", _I), ("summary", C.POINTER(VgxTrajSummaryIO)),
                ("form", C.c_int64), ("passes", C.c_int64), ("ms", C.c_double * 3)]


class VgxMilestonesIO(C.Structure):
    _fields_ = [("n", C.c_int64), ("replicates", _I), ("V", C.c_int64), ("variant_of", C.POINTER(C.c_int32)),
                ("K", C.c_int64), ("thresholds", C.POINTER(C.c_int32)),
                ("final", C.POINTER(C.c_int32)), ("peak", C.POINTER(C.c_int32)), ("peak_event", C.POINTER(C.c_int32)),
                ("last_positive_event", C.POINTER(C.c_int32)), ("first_event", C.POINTER(C.c_int32)),
                ("peak_time", _F), ("extinction_time", _F), ("first_time", _F),
                ("passes", C.c_int64), ("ms", C.c_double * 3)]


class VgxTauMilestonesIO(C.Structure):
    _fields_ = [("n", C.c_int64), ("replicates", _I), ("V", C.c_int64), ("variant_of", C.POINTER(C.c_int32)),
                ("K", C.c_int64), ("thresholds", _I),
                ("final", _I), ("peak", _I), ("peak_event", C.POINTER(C.c_int32)),
                ("last_positive_event", C.POINTER(C.c_int32)), ("first_event", C.POINTER(C.c_int32)),
                ("peak_time", _F), ("extinction_time", _F), ("first_time", _F),
                ("passes", C.c_int64), ("ms", C.c_double * 3)]


class VgxTauMilestonesChain(C.Structure):
    _fields_ = [("popNum", C.c_int64), ("hapNum", C.c_int64), ("ev_ptr", C.c_int64),
                ("ev_times", _F), ("ev_types", _I), ("ev_haplotypes", _I), ("ev_populations", _I),
                ("ev_newHaplotypes", _I), ("ev_newPopulations", _I),
                ("mev_rows", C.c_int64), ("mev_num", _I), ("mev_types", _I), ("mev_haplotypes", _I), ("mev_populations", _I),
                ("mev_newHaplotypes", _I), ("mev_newPopulations", _I),
                ("V", C.c_int64), ("variant_of", C.POINTER(C.c_int32)), ("start", _I), ("K", C.c_int64), ("thresholds", _I),
                ("tile", C.c_int64), ("n_own_events", C.c_int64), ("t_start", C.c_double),
                ("final", _I), ("peak", _I), ("peak_event", C.POINTER(C.c_int32)), ("last_positive_event", C.POINTER(C.c_int32)),
                ("first_event", C.POINTER(C.c_int32)), ("peak_time", _F), ("extinction_time", _F), ("first_time", _F)]


class VgxTauIncidenceIO(C.Structure):
    _fields_ = [("n", C.c_int64), ("replicates", _I), ("T", C.c_int64), ("edges", _F), ("hap_mask", C.POINTER(C.c_uint32)),
                ("counts", _I), ("outside", _I), ("summary", C.POINTER(VgxTrajSummaryIO)),
                ("passes", C.c_int64), ("ms", C.c_double * 3)]


class VgxTauIncidenceChain(C.Structure):
    _fields_ = [("popNum", C.c_int64), ("hapNum", C.c_int64), ("ev_ptr", C.c_int64),
                ("ev_times", _F), ("ev_types", _I), ("ev_haplotypes", _I), ("ev_populations", _I),
                ("ev_newHaplotypes", _I), ("ev_newPopulations", _I),
                ("mev_rows", C.c_int64), ("mev_num", _I), ("mev_types", _I), ("mev_haplotypes", _I), ("mev_populations", _I),
                ("mev_newHaplotypes", _I), ("mev_newPopulations", _I),
                ("T", C.c_int64), ("edges", _F), ("hap_mask", C.POINTER(C.c_uint32)), ("tile", C.c_int64), ("n_own_events", C.c_int64),
                ("counts", _I), ("outside", _I)]


class VgxTauFlowsIO(C.Structure):
    _fields_ = [("n", C.c_int64), ("replicates", _I), ("T", C.c_int64), ("edges", _F), ("V", C.c_int64), ("variant_of", C.POINTER(C.c_int32)),
                ("within", C.c_int32), ("counts", _I), ("outside", _I), ("summary", C.POINTER(VgxTrajSummaryIO)),
                ("form", C.c_int64), ("passes", C.c_int64), ("ms", C.c_double * 3)]


class VgxTauFlowsChain(C.Structure):
    _fields_ = [("popNum", C.c_int64), ("hapNum", C.c_int64), ("ev_ptr", C.c_int64),
                ("ev_times", _F), ("ev_types", _I), ("ev_haplotypes", _I), ("ev_populations", _I),
                ("ev_newHaplotypes", _I), ("ev_newPopulations", _I),
                ("mev_rows", C.c_int64), ("mev_num", _I), ("mev_types", _I), ("mev_haplotypes", _I), ("mev_populations", _I),
                ("mev_newHaplotypes", _I), ("mev_newPopulations", _I),
                ("T", C.c_int64), ("edges", _F), ("V", C.c_int64), ("variant_of", C.POINTER(C.c_int32)), ("within", C.c_int64),
                ("tile", C.c_int64), ("form", C.c_int64), ("n_own_events", C.c_int64), ("counts", _I), ("outside", _I),
                ("form_ran", C.c_int64)]


class VgxTauPrevalenceIO(C.Structure):
    _fields_ = [("n", C.c_int64), ("replicates", _I), ("T", C.c_int64), ("grid", _F), ("V", C.c_int64), ("variant_of", C.POINTER(C.c_int32)),
                ("values", _I), ("final", _I), ("outside", _I), ("summary", C.POINTER(VgxTrajSummaryIO)),
                ("passes", C.c_int64), ("ms", C.c_double * 3)]


class VgxTauPrevalenceChain(C.Structure):
    _fields_ = [("popNum", C.c_int64), ("hapNum", C.c_int64), ("ev_ptr", C.c_int64),
                ("ev_times", _F), ("ev_types", _I), ("ev_haplotypes", _I), ("ev_populations", _I),
                ("ev_newHaplotypes", _I), ("ev_newPopulations", _I),
                ("mev_rows", C.c_int64), ("mev_num", _I), ("mev_types", _I), ("mev_haplotypes", _I), ("mev_populations", _I),
                ("mev_newHaplotypes", _I), ("mev_newPopulations", _I),
                ("T", C.c_int64), ("grid", _F), ("V", C.c_int64), ("variant_of", C.POINTER(C.c_int32)), ("start", _I),
                ("tile", C.c_int64), ("n_own_events", C.c_int64), ("values", _I), ("final", _I), ("outside", _I)]


class VgxSusceptiblesIO(C.Structure):
    _fields_ = [("n", C.c_int64), ("replicates", _I), ("T", C.c_int64), ("grid", _F), ("G", C.c_int64), ("class_of", C.POINTER(C.c_int32)),
                ("values", C.POINTER(C.c_int32)), ("final", C.POINTER(C.c_int32)), ("outside", _I), ("summary", C.POINTER(VgxTrajSummaryIO)),
                ("passes", C.c_int64), ("ms", C.c_double * 3)]


class VgxTauSusceptiblesIO(C.Structure):
    _fields_ = [("n", C.c_int64), ("replicates", _I), ("T", C.c_int64), ("grid", _F), ("G", C.c_int64), ("class_of", C.POINTER(C.c_int32)),
                ("values", _I), ("final", _I), ("outside", _I), ("summary", C.POINTER(VgxTrajSummaryIO)),
                ("passes", C.c_int64), ("ms", C.c_double * 3)]


class VgxTauSusceptiblesChain(C.Structure):
    _fields_ = [("popNum", C.c_int64), ("susNum", C.c_int64), ("ev_ptr", C.c_int64),
                ("ev_times", _F), ("ev_types", _I), ("ev_haplotypes", _I), ("ev_populations", _I),
                ("ev_newHaplotypes", _I), ("ev_newPopulations", _I),
                ("mev_rows", C.c_int64), ("mev_num", _I), ("mev_types", _I), ("mev_haplotypes", _I), ("mev_populations", _I),
                ("mev_newHaplotypes", _I), ("mev_newPopulations", _I),
                ("T", C.c_int64), ("grid", _F), ("G", C.c_int64), ("class_of", C.POINTER(C.c_int32)), ("start", _I),
                ("tile", C.c_int64), ("n_own_events", C.c_int64), ("values", _I), ("final", _I), ("outside", _I)]


INCIDENCE_CHANNELS = ('birth', 'death', 'sampling', 'mutation', 'immunity', 'arrival', 'departure')   # vgx.h: channels 0 .. 6

COLSUMMARY_MAX_GROUP = 16384   # members of one group the device pass sorts (vgx.h: VGX_COLSUMMARY_MAX_GROUP)

TIMELINE_SEMANTICS = {'reference': 0, 'compartment': 1}


class VgxDirectShape(C.Structure):
    _fields_ = [(n, C.c_int64) for n in (
        "P", "H", "S", "sites", "R", "C", "CB", "cap", "n_seg", "n_solo_seg", "solo_npass0", "solo_npass1", "solo_ncls",
        "solo_maxnnz", "start_lone_rows", "start_max_nocc", "max_size", "hosts_below_2p53", "ld_possible", "recomb",
        "fresh_state", "suscep_cumul0_zero", "have_counts32", "tot_sus_is_sus", "no_lone", "solo_general", "param_sets")]


class VgxDirectPlan(C.Structure):
    _fields_ = [(n, C.c_int64) for n in (
        "kernel", "mode", "fast", "philox", "solo_mig_in_lds", "solo_compact", "lone_general", "lone_lds_bytes", "long_lists",
        "leaves32", "fallback_kernel", "fallback_mode")]


class VgxRowScan(C.Structure):
    _fields_ = [("rows", C.c_int64), ("H", C.c_int64), ("S", C.c_int64), ("infectious", _I), ("eventRates123", _F),
                ("numToHap", _I), ("bRate", _F), ("susceptibility", _F), ("rowSusceptible", _F), ("rowContact", _F), ("u", _F),
                ("birthRate", _F), ("tEvent", _F), ("hapPopRate", _F), ("susceptHapPopRate", _F), ("rowTotal", _F),
                ("chosen", _I), ("rnOut", _F)]


# every entry point include/vgx.h declares: (restype, argtypes)
_H = C.c_void_p
SIGNATURES = {
    "vgx_create": (C.c_int, [C.POINTER(VgxDims), C.c_int64, C.c_int, C.POINTER(_H)]),
    "vgx_destroy": (None, [_H]),
    "vgx_last_error": (C.c_char_p, [_H]),
    "vgx_device_count": (C.c_int, []),
    "vgx_set_params": (C.c_int, [_H, C.POINTER(VgxParams)]),
    "vgx_set_param_sets": (C.c_int, [_H, C.c_int64, C.POINTER(VgxParams), C.POINTER(C.c_int32)]),
    "vgx_set_recombination": (C.c_int, [_H, C.c_double, C.c_int64, _I]),
    "vgx_get_recombinations": (C.c_int, [_H, C.c_int64, C.c_int64, _I, _I, _I, _I, _I, _I]),
    "vgx_set_state": (C.c_int, [_H, C.POINTER(VgxState)]),
    "vgx_get_state": (C.c_int, [_H, C.c_int64, C.POINTER(VgxState)]),
    "vgx_set_seeds": (C.c_int, [_H, _I]),
    "vgx_stage_tau": (C.c_int, [_H]),
    "vgx_simulate_direct": (C.c_int, [_H, C.c_int64, C.c_int64, C.c_float, C.c_int64, C.POINTER(VgxRunOpts)]),
    "vgx_simulate_tau": (C.c_int, [_H, C.c_int64, C.c_int64, C.c_float, C.c_int64, C.POINTER(VgxRunOpts)]),
    "vgx_get_counters": (C.c_int, [_H, C.c_int64, C.POINTER(VgxCounters)]),
    "vgx_get_counters_all": (C.c_int, [_H, _I]),
    "vgx_get_events": (C.c_int, [_H, C.c_int64, C.c_int64, C.c_int64, _F, _I, _I, _I, _I, _I]),
    "vgx_get_lockdowns": (C.c_int, [_H, C.c_int64, C.c_int64, _I, _I, _F, _I]),
    "vgx_get_tau_tries": (C.c_int, [_H, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int32)]),
    "vgx_get_multievents": (C.c_int, [_H, C.c_int64, C.c_int64, _I, _F, _I, _I, _I, _I, _I, _I]),
    "vgx_get_multievents_all": (C.c_int, [_H, C.c_int64, _I, _I, _I]),
    "vgx_get_tau_states_all": (C.c_int, [_H, _I, _I, _I, _F]),
    "vgx_get_trajectories": (C.c_int, [_H, C.c_void_p, C.c_int]),
    "vgx_get_trajectories_int": (C.c_int, [_H, C.c_void_p]),
    "vgx_get_trajectory_summary": (C.c_int, [_H, C.POINTER(VgxTrajSummaryIO)]),
    "vgx_test_column_summary": (C.c_int, [_F, C.c_int64, C.c_int64, C.POINTER(VgxTrajSummaryIO), C.c_char_p, C.c_int64]),
    "vgx_clock_mismatches": (C.c_int64, [_H]),
    "vgx_last_kernel_ms": (C.c_double, [_H]),
    "vgx_last_kernel_launches": (C.c_int64, [_H]),
    "vgx_last_direct_kernel": (C.c_int, [_H]),
    "vgx_device_bytes": (C.c_int64, [_H]),
    "vgx_get_profile": (C.c_int, [_H, C.c_int64, _I]),
    "vgx_get_list_counts_quad": (C.c_int, [_H, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int32), _I]),
    "vgx_get_list_tile_sums": (C.c_int, [_H, C.c_int64, C.c_int64, C.c_int64, _I, _I]),
    "vgx_get_genealogy": (C.c_int, [C.POINTER(VgxGenealogyIO), C.c_char_p, C.c_int64]),
    "vgx_get_genealogies": (C.c_int, [_H, C.POINTER(VgxGenealogiesIO)]),
    "vgx_genealogy_message": (C.c_int, [C.c_int64, C.c_int64, C.c_char_p, C.c_int64]),
    "vgx_test_genealogy_walk": (C.c_int, [C.POINTER(VgxGenealogyIO), C.c_char_p, C.c_int64]),
    "vgx_get_tau_genealogies": (C.c_int, [_H, C.POINTER(VgxTauGenealogiesIO), C.POINTER(VgxTauGenealogyPrefix)]),
    "vgx_test_tau_genealogy_walk": (C.c_int, [C.POINTER(VgxGenealogyIO), C.c_int64, C.c_char_p, C.c_int64]),
    "vgx_test_hypergeometric": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_uint64 * 6), _I]),
    "vgx_get_timelines": (C.c_int, [_H, C.POINTER(VgxTimelinesIO)]),
    "vgx_test_timelines": (C.c_int, [C.POINTER(VgxTimelinesChain), C.c_char_p, C.c_int64]),
    "vgx_get_tau_timelines": (C.c_int, [_H, C.POINTER(VgxTimelinesIO), C.POINTER(VgxTimelinesPrefix)]),
    "vgx_test_tau_timelines": (C.c_int, [C.POINTER(VgxTauTimelinesChain), C.c_char_p, C.c_int64]),
    "vgx_get_incidence": (C.c_int, [_H, C.POINTER(VgxIncidenceIO)]),
    "vgx_test_incidence": (C.c_int, [_F, _I, _I, _I, _I, _I, C.c_int64, C.c_int64, C.c_int64, _F, C.c_int64, C.POINTER(C.c_uint32), C.c_int64,
                                     C.POINTER(C.c_int32), _I, C.c_char_p, C.c_int64]),
    "vgx_get_prevalence": (C.c_int, [_H, C.POINTER(VgxPrevalenceIO)]),
    "vgx_test_prevalence": (C.c_int, [_F, _I, _I, _I, _I, _I, C.c_int64, C.c_int64, C.c_int64, _F, C.c_int64, C.POINTER(C.c_int32), C.c_int64, _I,
                                      C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, C.c_char_p, C.c_int64]),
    "vgx_get_lineages": (C.c_int, [_H, C.POINTER(VgxLineagesIO)]),
    "vgx_test_lineages": (C.c_int, [C.POINTER(VgxGenealogyIO), _F, C.c_int64, C.POINTER(C.c_int32), C.c_int64, C.c_int64, C.POINTER(C.c_int32),
                                    C.POINTER(C.c_int32), _I, C.c_char_p, C.c_int64]),
    "vgx_get_tau_lineages": (C.c_int, [_H, C.POINTER(VgxTauLineagesIO), C.POINTER(VgxTauGenealogyPrefix)]),
    "vgx_test_tau_lineages": (C.c_int, [C.POINTER(VgxGenealogyIO), C.c_int64, _F, C.c_int64, C.POINTER(C.c_int32), C.c_int64, C.c_int64,
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, C.c_char_p, C.c_int64]),
    "vgx_get_tree_events": (C.c_int, [_H, C.POINTER(VgxTreeEventsIO)]),
    "vgx_test_tree_events": (C.c_int, [C.POINTER(VgxGenealogyIO), _F, C.c_int64, C.POINTER(C.c_int32), C.c_int64, C.c_int64, C.POINTER(C.c_int32),
                                       _I, C.c_char_p, C.c_int64]),
    "vgx_get_tau_tree_events": (C.c_int, [_H, C.POINTER(VgxTauTreeEventsIO), C.POINTER(VgxTauGenealogyPrefix)]),
    "vgx_test_tau_tree_events": (C.c_int, [C.POINTER(VgxGenealogyIO), C.c_int64, _F, C.c_int64, C.POINTER(C.c_int32), C.c_int64, C.c_int64,
                                           C.POINTER(C.c_int32), _I, C.c_char_p, C.c_int64]),
    "vgx_get_tree_shapes": (C.c_int, [_H, C.POINTER(VgxTreeShapesIO)]),
    "vgx_test_tree_shape": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), _F, C.c_int64, _I, _F, C.c_char_p, C.c_int64]),
    "vgx_test_tree_shape_device": (C.c_int, [C.c_int64, _I, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _F, _I, _F, _I, C.c_char_p, C.c_int64]),
    "vgx_get_tau_tree_shapes": (C.c_int, [_H, C.POINTER(VgxTauTreeShapesIO), C.POINTER(VgxTauGenealogyPrefix)]),
    "vgx_get_mutation_spectrum": (C.c_int, [_H, C.POINTER(VgxMutationSpectrumIO)]),
    "vgx_get_tau_mutation_spectrum": (C.c_int, [_H, C.POINTER(VgxTauMutationSpectrumIO), C.POINTER(VgxTauGenealogyPrefix)]),
    "vgx_test_mutation_spectrum": (C.c_int, [C.POINTER(C.c_int32), C.c_int64] + [C.POINTER(C.c_int32)] * 4 + [C.c_int64, C.c_int64, _I, _I, _I, _I,
                                             C.POINTER(C.c_int32), C.c_char_p, C.c_int64]),
    "vgx_test_mutation_spectrum_device": (C.c_int, [C.c_int64, _I, C.POINTER(C.c_int32), _I] + [C.POINTER(C.c_int32)] * 4 +
                                          [C.c_int64, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_int32), C.c_char_p, C.c_int64]),
    "vgx_get_introductions": (C.c_int, [_H, C.POINTER(VgxIntroductionsIO)]),
    "vgx_get_tau_introductions": (C.c_int, [_H, C.POINTER(VgxTauIntroductionsIO), C.POINTER(VgxTauGenealogyPrefix)]),
    "vgx_test_introductions": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int64, C.c_int64, _I, _I, _I, _I, _I,
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_char_p, C.c_int64]),
    "vgx_test_introductions_device": (C.c_int, [C.c_int64, _I, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int64, _I, _I, _I, _I, _I, _I, _I,
                                                C.c_char_p, C.c_int64]),
    "vgx_test_tau_node_times": (C.c_int, [C.POINTER(C.c_int32), C.c_int64, C.c_int64, _F, C.c_int64, _F, _F, C.c_char_p, C.c_int64]),
    "vgx_test_tau_node_times_device": (C.c_int, [C.c_int64, _I, C.POINTER(C.c_int32), _I, C.c_int64, _F, _I, _F, _F, C.POINTER(C.c_int32),
                                                 C.c_char_p, C.c_int64]),
    "vgx_get_flows": (C.c_int, [_H, C.POINTER(VgxFlowsIO)]),
    "vgx_test_flows": (C.c_int, [_F, _I, _I, _I, _I, _I, C.c_int64, C.c_int64, C.c_int64, _F, C.c_int64, C.POINTER(C.c_int32), C.c_int64, C.c_int32,
                                 C.c_int64, C.c_int64, C.POINTER(C.c_int32), _I, _I, C.c_char_p, C.c_int64]),
    "vgx_get_milestones": (C.c_int, [_H, C.POINTER(VgxMilestonesIO)]),
    "vgx_test_milestones": (C.c_int, [_F, _I, _I, _I, _I, _I, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.c_int64, _I,
                                      C.POINTER(C.c_int32), C.c_int64, C.c_int64, C.c_double] + [C.POINTER(C.c_int32)] * 5 + [_F] * 3 +
                            [C.c_char_p, C.c_int64]),
    "vgx_get_tau_milestones": (C.c_int, [_H, C.POINTER(VgxTauMilestonesIO), C.POINTER(VgxTimelinesPrefix)]),
    "vgx_test_tau_milestones": (C.c_int, [C.POINTER(VgxTauMilestonesChain), C.c_char_p, C.c_int64]),
    "vgx_get_tau_incidence": (C.c_int, [_H, C.POINTER(VgxTauIncidenceIO), C.POINTER(VgxTimelinesPrefix)]),
    "vgx_test_tau_incidence": (C.c_int, [C.POINTER(VgxTauIncidenceChain), C.c_char_p, C.c_int64]),
    "vgx_get_tau_flows": (C.c_int, [_H, C.POINTER(VgxTauFlowsIO), C.POINTER(VgxTimelinesPrefix)]),
    "vgx_test_tau_flows": (C.c_int, [C.POINTER(VgxTauFlowsChain), C.c_char_p, C.c_int64]),
    "vgx_get_tau_prevalence": (C.c_int, [_H, C.POINTER(VgxTauPrevalenceIO), C.POINTER(VgxTimelinesPrefix)]),
    "vgx_test_tau_prevalence": (C.c_int, [C.POINTER(VgxTauPrevalenceChain), C.c_char_p, C.c_int64]),
    "vgx_get_susceptibles": (C.c_int, [_H, C.POINTER(VgxSusceptiblesIO)]),
    "vgx_test_susceptibles": (C.c_int, [_F, _I, _I, _I, _I, _I, C.c_int64, C.c_int64, C.c_int64, _F, C.c_int64, C.POINTER(C.c_int32), C.c_int64, _I,
                                        C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, C.c_char_p, C.c_int64]),
    "vgx_get_tau_susceptibles": (C.c_int, [_H, C.POINTER(VgxTauSusceptiblesIO), C.POINTER(VgxTimelinesPrefix)]),
    "vgx_test_tau_susceptibles": (C.c_int, [C.POINTER(VgxTauSusceptiblesChain), C.c_char_p, C.c_int64]),
    "vgx_test_direct_plan": (C.c_int, [C.POINTER(VgxDirectShape), C.POINTER(VgxRunOpts), C.POINTER(VgxDirectPlan), C.c_char_p, C.c_int64]),
    "vgx_rng_position": (None, [C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_uint64 * 4)]),
    "vgx_propensity_scan": (C.c_int, [C.POINTER(VgxRowScan)]),
    "vgx_propensity_scan_bench": (C.c_int, [C.POINTER(VgxRowScan), C.c_int64, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "vgx_propensity_scan_error": (C.c_char_p, []),
    "vgx_test_philox": (C.c_int, [C.c_int, C.POINTER(C.c_uint32 * 4), C.POINTER(C.c_uint32 * 2), C.POINTER(C.c_uint32 * 4)]),
    "vgx_test_poisson": (C.c_int, [C.c_double, C.c_int64, C.c_uint64, _I]),
    "vgx_test_div_by_const": (C.c_int, [_F, _F, C.c_int64, _F, _F, _F]),
    "vgx_test_row_scans": (C.c_int, [_F, _F, C.c_int64, _F, _F, _F]),
    "vgx_test_quad_tile_choice": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _F, _F, C.c_int64, C.c_int64, C.c_int,
                                            C.POINTER(C.c_int32), _F, _F, _I]),
}

_lib = None


def load_library():
    """Load libvgx.so and bind every symbol of include/vgx.h; raises if the HIP extension is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "vgsim_amd: the HIP extension %s is not built (run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C vgsim_amd/csrc`). There is no CPU fallback." % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _p(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    if a.dtype == np.float64:
        return a.ctypes.data_as(_F)
    if a.dtype == np.int64:
        return a.ctypes.data_as(_I)
    raise TypeError(a.dtype)


class VgxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libvgx error %d: %s" % (code, msg))
        self.code = code


class HipEngine:
    """One libvgx engine: a model shape and ``n_replicates`` independent seeded trajectories on one GPU."""

    def __init__(self, sites, hapNum, popNum, susNum, n_replicates=1, device=0):
        self.lib = load_library()
        self.dims = VgxDims(sites, hapNum, popNum, susNum)
        self.R = int(n_replicates)
        self.handle = _H()
        rc = self.lib.vgx_create(C.byref(self.dims), self.R, int(device), C.byref(self.handle))
        if rc != VGX_OK:
            self.handle = None
            raise VgxError(rc, self.lib.vgx_last_error(None).decode())
        self.P, self.H, self.S = popNum, hapNum, susNum

    def close(self):
        if getattr(self, "handle", None):
            self.lib.vgx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != VGX_OK:
            raise VgxError(rc, self.lib.vgx_last_error(self.handle).decode())

    # ---------------------------------------------------------------- hand-over
    @staticmethod
    def _fill_params(p, m):
        """The pointers of a ``VgxParams`` from host model ``m``; returns the arrays they refer to (contiguous, of the declared
        dtype), which must stay alive until the library call returns."""
        conv = []
        for name, ctype in VgxParams._fields_:
            a = np.ascontiguousarray(getattr(m, name), dtype=np.int64 if ctype is _I else np.float64)
            conv.append(a)
            setattr(p, name, _p(a))
        return conv

    def set_params(self, m):
        p = VgxParams()
        self._keep = self._fill_params(p, m)
        self._check(self.lib.vgx_set_params(self.handle, C.byref(p)))
        self._set_recombination(m)

    def set_param_sets(self, models, set_of):
        """Scenario ensembles (``vgx_set_param_sets``): replicate r runs under the parameters of ``models[set_of[r]]``.
        Recombination settings are those of ``models[0]`` (shared by all sets)."""
        sets = (VgxParams * len(models))()
        keep, filled = [], {}
        for g, m in enumerate(models):
            if id(m) in filled:        # the same model object given again: the same arrays
                sets[g] = sets[filled[id(m)]]
                continue
            filled[id(m)] = g
            keep.append(self._fill_params(sets[g], m))
        of = np.ascontiguousarray(set_of, dtype=np.int32)
        assert of.shape == (self.R,)
        self._keep = keep
        self._check(self.lib.vgx_set_param_sets(self.handle, len(models), sets, of.ctypes.data_as(C.POINTER(C.c_int32))))
        self._set_recombination(models[0])

    def _set_recombination(self, m):
        pos = np.ascontiguousarray(getattr(m, "sitesPosition", np.zeros(0)), dtype=np.int64)
        self._check(self.lib.vgx_set_recombination(self.handle, float(getattr(m, "recombination", 0.0)),
                                                   int(getattr(m, "genome_length", 0)), _p(pos) if len(pos) else None))

    def recombinations(self, replicate=0):
        """Forward recombination records of the last direct call: (idevents, his, hi2s, nhis, posRecombs)."""
        n = C.c_int64(0)
        self._check(self.lib.vgx_get_recombinations(self.handle, replicate, 0, None, None, None, None, None, C.byref(n)))
        cols = [np.zeros(n.value, dtype=np.int64) for _ in range(5)]
        if n.value:
            self._check(self.lib.vgx_get_recombinations(self.handle, replicate, n.value, *[_p(c) for c in cols], C.byref(n)))
        return cols

    def _state_struct(self, m):
        s = VgxState()
        for name in ("susceptible", "infectious", "initial_susceptible", "initial_infectious", "totalSusceptible",
                     "totalInfectious", "lockdownON", "contactDensity"):
            setattr(s, name, _p(getattr(m, name)))
        return s

    def set_state(self, m):
        s = self._state_struct(m)
        s.first_simulation = int(m.first_simulation)
        s.globalInfectious = int(m.globalInfectious)
        for c in m.COUNTERS + ("good_attempt",):
            setattr(s, c, int(getattr(m, c)))
        s.currentTime, s.totalRate, s.totalMigrationRate, s.tau_l = m.currentTime, m.totalRate, m.totalMigrationRate, m.tau_l
        s.ev_ptr, s.ev_size = m.events.ptr, m.events.size
        # upstream's first_simulation is False until the first simulation (pyx:76, 435-448): the call after this one snapshots the
        # initial state exactly then, and get_state reads it back after that call only
        self._snapshot_call = not bool(m.first_simulation)
        self._check(self.lib.vgx_set_state(self.handle, C.byref(s)))

    def get_state(self, m, replicate=0):
        s = self._state_struct(m)
        if not getattr(self, "_snapshot_call", True):
            # the initial state is written by the first simulation's snapshot alone (pyx:419-424): at config 4's size copying it back
            # after every call is 2 GB of memcpy for nothing
            s.initial_susceptible = None
            s.initial_infectious = None
        self._check(self.lib.vgx_get_state(self.handle, replicate, C.byref(s)))
        m.first_simulation = bool(s.first_simulation)
        m.globalInfectious = s.globalInfectious
        for c in m.COUNTERS + ("good_attempt",):
            setattr(m, c, getattr(s, c))
        m.currentTime, m.totalRate, m.totalMigrationRate, m.tau_l = s.currentTime, s.totalRate, s.totalMigrationRate, s.tau_l

    def stage_tau(self):
        """Put the state of the last ``set_state`` on the device in the tau kernels' layout now (``vgx_stage_tau``): the next
        ``vgx_simulate_tau`` then starts from resident inputs."""
        self._check(self.lib.vgx_stage_tau(self.handle))

    def set_seeds(self, seeds):
        a = np.ascontiguousarray(np.asarray(seeds, dtype=np.int64))
        assert a.shape == (self.R,)
        self._check(self.lib.vgx_set_seeds(self.handle, _p(a)))

    def counters(self, replicate=0):
        c = VgxCounters()
        self._check(self.lib.vgx_get_counters(self.handle, replicate, C.byref(c)))
        return c

    def fetch_events(self, events, replicate, first, count):
        """Copy device log rows [first, first+count) into a host ``Events`` object at the same indices."""
        if count <= 0:
            return
        sl = slice(first, first + count)
        bufs = [np.zeros(count, dtype=np.float64)] + [np.zeros(count, dtype=np.int64) for _ in range(5)]
        self._check(self.lib.vgx_get_events(self.handle, replicate, first, count, *[_p(b) for b in bufs]))
        events.times[sl] = bufs[0]
        for name, b in zip(events.COLUMNS, bufs[1:]):
            getattr(events, name)[sl] = b

    def lockdowns(self, replicate=0, cap=4096):
        st, pp = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int64)
        tt = np.zeros(cap, dtype=np.float64)
        n = C.c_int64(0)
        self._check(self.lib.vgx_get_lockdowns(self.handle, replicate, cap, _p(st), _p(pp), _p(tt), C.byref(n)))
        k = min(n.value, cap)
        return st[:k], pp[:k], tt[:k]

    # ---------------------------------------------------------------- the hot path for one host model
    def simulate_direct(self, m, iterations, sample_size, time, attempts, opts=None):
        """``BirthDeathModel.SimulatePopulation`` (pyx:396-429) for a host model object: upload, run the
        persistent kernel, read the model back exactly as the reference would leave it."""
        self.set_params(m)
        self.set_state(m)
        self.set_seeds([m.user_seed] * self.R)
        rc = self.lib.vgx_simulate_direct(self.handle, iterations, sample_size, float(time), attempts,
                                          C.byref(opts) if opts is not None else None)
        self._check(rc)
        self._absorb(m)

    def simulate_tau(self, m, iterations, sample_size, time, attempts, opts=None):
        """``BirthDeathModel.SimulatePopulation_tau`` (pyx:2293-2346)."""
        self.set_params(m)
        self.set_state(m)
        self.set_seeds([m.user_seed] * self.R)
        rc = self.lib.vgx_simulate_tau(self.handle, iterations, sample_size, float(time), attempts,
                                       C.byref(opts) if opts is not None else None)
        self._check(rc)
        mev_base = m.multievents.ptr   # rows of earlier tau calls stay in the log
        self._absorb(m, tau=True, mev_base=mev_base)

    def multievents(self, replicate=0):
        """Rows (num > 0 only) of the last tau call: dict of arrays num, times, types, haplotypes, ..."""
        n = C.c_int64(0)
        self._check(self.lib.vgx_get_multievents(self.handle, replicate, 0, None, None, None, None, None, None, None, C.byref(n)))
        k = n.value
        cols = {name: np.zeros(k, dtype=np.int64) for name in ("num", "types", "haplotypes", "populations", "newHaplotypes", "newPopulations")}
        times = np.zeros(k, dtype=np.float64)
        if k:
            self._check(self.lib.vgx_get_multievents(self.handle, replicate, k, _p(cols["num"]), _p(times), _p(cols["types"]),
                                                     _p(cols["haplotypes"]), _p(cols["populations"]), _p(cols["newHaplotypes"]),
                                                     _p(cols["newPopulations"]), C.byref(n)))
        cols["times"] = times
        return cols

    def multievents_all(self):
        """The rows of every replicate of the last tau call in one read-out (``vgx_get_multievents_all``): ``offsets`` [R + 1] and a dict
        of arrays (num, types, haplotypes, populations, newHaplotypes, newPopulations, steps) in which rows offsets[r]:offsets[r + 1]
        are replicate r's, in the device's order (``canonical_multievents`` gives the reference's)."""
        off = np.zeros(self.R + 1, dtype=np.int64)
        self._check(self.lib.vgx_get_multievents_all(self.handle, 0, _p(off), None, None))
        n = int(off[-1])
        rows = np.zeros((max(n, 1), 6), dtype=np.int64)
        steps = np.zeros(max(n, 1), dtype=np.int64)
        if n:
            self._check(self.lib.vgx_get_multievents_all(self.handle, n, _p(off), _p(rows), _p(steps)))
        cols = {name: np.ascontiguousarray(rows[:n, j]) for j, name in enumerate(("num", "types", "haplotypes", "populations", "newHaplotypes", "newPopulations"))}
        cols["steps"] = steps[:n]
        return off, cols

    def tau_states_all(self):
        """infectious [R, P, H], susceptible [R, P, S], counters [R, 8] (bCounter, dCounter, sCounter, mCounter, iCounter, migPlus,
        globalInfectious, ev_ptr) and currentTime [R] of every replicate after the last tau call (``vgx_get_tau_states_all``)."""
        inf = np.zeros((self.R, self.P, self.H), dtype=np.int64)
        sus = np.zeros((self.R, self.P, self.S), dtype=np.int64)
        cnt = np.zeros((self.R, 8), dtype=np.int64)
        t = np.zeros(self.R, dtype=np.float64)
        self._check(self.lib.vgx_get_tau_states_all(self.handle, _p(inf), _p(sus), _p(cnt), _p(t)))
        return inf, sus, cnt, t

    def counters_all(self):
        """``[R, 4]`` int64: ev_ptr, loop_iterations, restarts, tau events drawn of every replicate."""
        out = np.zeros((self.R, 4), dtype=np.int64)
        self._check(self.lib.vgx_get_counters_all(self.handle, _p(out)))
        return out

    def _absorb(self, m, replicate=0, tau=False, mev_base=0):
        self.get_state(m, replicate)
        c = self.counters(replicate)
        first = c.ev_first_new
        self.fetch_events(m.events, replicate, first, c.ev_ptr - first)
        m.events.ptr = c.ev_ptr
        if tau:
            rows = self.multievents(replicate)
            if len(rows["times"]) == 0:    # nothing recorded (record_multievents=False or no event drawn): empty row ranges
                m.events.haplotypes[first:c.ev_ptr] = 0
                m.events.populations[first:c.ev_ptr] = 0
            rows = canonical_multievents(rows, m.events.haplotypes[first:c.ev_ptr], m.events.populations[first:c.ev_ptr],
                                         m.sites, m.susNum)
            if c.restarts > 0:  # Restart rewinds multievents.ptr too (pyx:716)
                m.multievents.ptr = 0
                mev_base = 0
            # MULTITYPE records carry the [start, end) range of their rows (pyx:2325), here within the sparse log
            m.events.haplotypes[first:c.ev_ptr] += mev_base
            m.events.populations[first:c.ev_ptr] += mev_base
            m.multievents.extend(rows.pop("times"), **rows)
            self.last_events_drawn = c.reserved[0]
        st, pp, tt = self.lockdowns(replicate)
        for k in range(len(st)):
            m.loc.AddLockdown(st[k], pp[k], tt[k])
        if not tau and getattr(m, "recombination", 0.0) and hasattr(m, "rec"):
            for row in zip(*self.recombinations(replicate)):
                m.rec.AddRecombination_forward(*row)
        self.last_counters = c

    def tau_tries(self, replicate, first, count):
        """Rejected tries (halvings of tau_l, pyx:2316-2321) of steps [first, first + count) of the last tau call."""
        out = np.zeros(count, dtype=np.int32)
        self._check(self.lib.vgx_get_tau_tries(self.handle, replicate, first, count, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    @property
    def last_kernel_ms(self):
        return self.lib.vgx_last_kernel_ms(self.handle)

    @property
    def last_kernel(self):
        """Name of the kernel the last direct call ran on (vgx_run_opts.kernel)."""
        return {1: "wave", 2: "lane", 3: "quad", 4: "quadg", 5: "solo", 6: "lone"}[self.lib.vgx_last_direct_kernel(self.handle)]

    @property
    def device_bytes(self):
        return self.lib.vgx_device_bytes(self.handle)


def canonical_multievents(rows, starts, ends, sites, susNum):
    """Rows of one tau call in the reference's order and granularity.  The device appends a step's rows in whatever
    order its threads get there (and one row per drawn transmission / mutant / migrant); the reference writes one row
    per channel in a fixed order (UpdateCompartmentCounts_tau, pyx:2540-2593: all migrations by (source, target,
    group, haplotype); then per population the immunity transitions, then per haplotype recovery, sampling, mutations
    by (site, derived state), transmissions by group).  Sorting each step's rows by that key and merging equal channels
    gives the reference's rows with ``num > 0`` — what the backward pass (pyx:873-994) walks — independent of
    scheduling.  ``starts`` / ``ends`` (the MULTITYPE events' row ranges, relative to this call) are updated in place."""
    n = len(rows["times"])
    if n == 0:
        return rows
    num, typ, hap = rows["num"], rows["types"], rows["haplotypes"]
    pop, nh, npop = rows["populations"], rows["newHaplotypes"], rows["newPopulations"]
    step = np.searchsorted(np.asarray(ends), np.arange(n), side="right")
    mig = typ == 5
    k1 = np.where(mig, 0, 1)
    k2 = pop.copy()                                  # source population / population
    k3 = np.where(mig, npop, np.where(typ == 4, 0, 1))
    k4 = np.where(mig, nh, hap)                      # migration: group; else source group / haplotype
    k5 = np.zeros(n, dtype=np.int64)
    k5[mig] = hap[mig]
    k5[typ == 4] = nh[typ == 4]
    k5[typ == 1] = 0
    k5[typ == 2] = 1
    mu = typ == 3
    if mu.any():
        d = np.abs(nh[mu] - hap[mu])
        low = np.zeros(d.shape, dtype=np.int64)      # digit position from the least significant end
        t = d.copy()
        while (t >= 4).any():
            big = t >= 4
            t[big] //= 4
            low[big] += 1
        digit4 = 4 ** low
        AS, DS = (hap[mu] // digit4) % 4, (nh[mu] // digit4) % 4
        k5[mu] = 2 + (sites - 1 - low) * 3 + np.where(DS > AS, DS - 1, DS)
    k5[typ == 0] = 2 + 3 * sites + nh[typ == 0]
    order = np.lexsort((k5, k4, k3, k2, k1, step))
    key = np.stack([step, k1, k2, k3, k4, k5])[:, order]
    first = np.ones(n, dtype=bool)
    first[1:] = (key[:, 1:] != key[:, :-1]).any(axis=0)
    idx = np.nonzero(first)[0]
    out = {c: rows[c][order][idx] for c in ("types", "haplotypes", "populations", "newHaplotypes", "newPopulations")}
    out["num"] = np.add.reduceat(num[order], idx)
    out["times"] = rows["times"][order][idx]
    per_step = np.bincount(key[0, idx], minlength=len(starts))
    e = np.cumsum(per_step)
    starts[:] = e - per_step
    ends[:] = e
    return out


def get_genealogy(m, seed=None, rng_position=None, rng_raw=None):
    """``BirthDeathModel.GetGenealogy(seed)`` (pyx:743-1000) on a host model: the backward pass over ``m.events`` (and
    ``m.multievents`` for tau chains) in libvgx's host code.  ``seed``: reseeds the stream as the reference does
    (``RndmWrapper(seed=(seed, 0))``, pyx:766-767); ``None`` continues from ``rng_position`` = (attempt, draws) of the
    simulation's stream, or from ``rng_raw`` = the raw generator state a previous pass returned (``out["rng_raw"]``).
    Walks ``m.infectious`` back in place; returns a dict of arrays."""
    return _genealogy("vgx_get_genealogy", m, seed, rng_position, rng_raw)


def genealogy_walk(m, seed=None, rng_position=None, rng_raw=None):
    """``get_genealogy`` through ``vgx_test_genealogy_walk``: the walk of the device pass (vgx_gwalk.h) compiled for the
    host, on the same arguments (direct chains only).  Same dict, same exceptions."""
    return _genealogy("vgx_test_genealogy_walk", m, seed, rng_position, rng_raw)


def tau_genealogy_walk(m, seed=None, rng_position=None, rng_raw=None):
    """``get_genealogy`` through ``vgx_test_tau_genealogy_walk``: the walk of the device pass for tau chains (vgx_gwalk_tau.h)
    compiled for the host, on the same arguments.  The chain's trailing MULTITYPE events play a replicate's own steps: their
    rows may come in any order and granularity; everything before them is taken as it is.  Same dict, same exceptions."""
    return _genealogy("vgx_test_tau_genealogy_walk", m, seed, rng_position, rng_raw, extra=(int(m.sites),))


def hypergeometric(good, bad, sample, n, state, on_device=False):
    """``n`` draws of numpy's ``random_hypergeometric(good, bad, sample)`` by the sampler of the tau walk (``vgx_test_hypergeometric``;
    the host build, or the device's).  ``state``: PCG64 state hi, lo, increment hi, lo, has_uint32, uinteger.  Returns (draws, state
    after them)."""
    st = (C.c_uint64 * 6)(*[int(x) for x in state])
    out = np.zeros(max(int(n), 1), dtype=np.int64)
    rc = load_library().vgx_test_hypergeometric(1 if on_device else 0, int(good), int(bad), int(sample), int(n), C.byref(st), _p(out))
    if rc != VGX_OK:
        raise VgxError(rc, "vgx_test_hypergeometric failed")
    return out[:n], tuple(int(x) for x in st)


def genealogy_message(status, arg):
    """The text ``vgx_get_genealogy`` reports for a walk status of ``vgx_get_genealogies``."""
    buf = C.create_string_buffer(512)
    load_library().vgx_genealogy_message(int(status), int(arg), buf, 512)
    return buf.value.decode()


def _genealogy_chain(m, seed, rng_position, rng_raw):
    """A ``VgxGenealogyIO`` with the chain, the state and the generator start of a host model, its outputs not yet allocated:
    (io, MUTATION events, MIGRATION events of the chain, multievent rows weighted)."""
    lib = load_library()
    ev, mv = m.events, m.multievents
    io = VgxGenealogyIO()
    io.popNum, io.hapNum, io.sCounter, io.ev_ptr = m.popNum, m.hapNum, int(m.sCounter), int(ev.ptr)
    io.ev_times, io.ev_types, io.ev_haplotypes = _p(ev.times), _p(ev.types), _p(ev.haplotypes)
    io.ev_populations, io.ev_newHaplotypes, io.ev_newPopulations = _p(ev.populations), _p(ev.newHaplotypes), _p(ev.newPopulations)
    types = ev.types[:ev.ptr]
    n_mut, n_mig = int((types == 3).sum()), int((types == 5).sum())
    if mv.ptr > 0:
        io.mev_rows = int(mv.ptr)
        io.mev_num, io.mev_times, io.mev_types = _p(mv.num), _p(mv.times), _p(mv.types)
        io.mev_haplotypes, io.mev_populations = _p(mv.haplotypes), _p(mv.populations)
        io.mev_newHaplotypes, io.mev_newPopulations = _p(mv.newHaplotypes), _p(mv.newPopulations)
        n_mut += int(mv.num[:mv.ptr][mv.types[:mv.ptr] == 3].sum())
        n_mig += int(mv.num[:mv.ptr][mv.types[:mv.ptr] == 5].sum())
    if not m.infectious.flags["C_CONTIGUOUS"]:
        raise ValueError("infectious must be C-contiguous")
    io.infectious = _p(m.infectious)
    pos = (C.c_uint64 * 4)()
    if seed is not None:
        lib.vgx_rng_position(int(seed), 0, 0, C.byref(pos))
    elif rng_raw is not None:
        for i in range(4):
            pos[i] = rng_raw[i]
        io.rng_has_uint32, io.rng_uinteger = int(rng_raw[4]), int(rng_raw[5])
    else:
        att, draws = rng_position if rng_position is not None else (0, 0)
        lib.vgx_rng_position(int(m.user_seed), int(att), int(draws), C.byref(pos))
    for i in range(4):
        io.rng_state[i] = pos[i]
    return io, n_mut, n_mig


def _genealogy(entry, m, seed, rng_position, rng_raw, extra=()):
    lib = load_library()
    io, n_mut, n_mig = _genealogy_chain(m, seed, rng_position, rng_raw)
    nodes = max(2 * int(m.sCounter) - 1, 1)
    out = {"tree": np.zeros(nodes, dtype=np.int64), "tree_pop": np.zeros(nodes, dtype=np.int64), "times": np.zeros(nodes)}
    io.tree, io.tree_pop, io.times = _p(out["tree"]), _p(out["tree_pop"]), _p(out["times"])
    io.mut_cap, io.mig_cap = n_mut + 1, n_mig + nodes + 1
    for k in ("mut_node", "mut_AS", "mut_DS", "mut_site"):
        out[k] = np.zeros(io.mut_cap, dtype=np.int64)
        setattr(io, k, _p(out[k]))
    out["mut_time"] = np.zeros(io.mut_cap)
    io.mut_time = _p(out["mut_time"])
    for k in ("mig_node", "mig_old", "mig_new"):
        out[k] = np.zeros(io.mig_cap, dtype=np.int64)
        setattr(io, k, _p(out[k]))
    out["mig_time"] = np.zeros(io.mig_cap)
    io.mig_time = _p(out["mig_time"])
    err = C.create_string_buffer(512)
    rc = getattr(lib, entry)(C.byref(io), *extra, err, 512)
    if rc != 0:
        raise RuntimeError(err.value.decode() or "%s failed (%d)" % (entry, rc))
    for k in list(out):
        if k.startswith("mut_"):
            out[k] = out[k][:io.mut_n]
        elif k.startswith("mig_"):
            out[k] = out[k][:io.mig_n]
    out["nodes_used"] = int(io.nodes_used)
    out["rng_raw"] = tuple(int(io.rng_state[i]) for i in range(4)) + (int(io.rng_has_uint32), int(io.rng_uinteger))
    return out


def unique_queries(pairs):
    """(unique pairs as an (k, 2) int64 array in first-seen order, index of every given pair among them)."""
    seen, uniq, index = {}, [], []
    for a, b in pairs:
        key = (int(a), int(b))
        if key not in seen:
            seen[key] = len(uniq)
            uniq.append(key)
        index.append(seen[key])
    return np.asarray(uniq, dtype=np.int64).reshape(-1, 2), np.asarray(index, dtype=np.int64)


def _timelines_chain(m, infectious, susceptible, step_num, semantics):
    """A ``VgxTimelinesChain`` for host model ``m`` with its outputs allocated: (io, finish) where ``finish()`` gives the result dict."""
    if semantics not in TIMELINE_SEMANTICS:
        raise ValueError("semantics must be 'reference' or 'compartment'")
    ev = m.events
    qi, ii = unique_queries(infectious)
    qs, si = unique_queries(susceptible)
    T = int(step_num) + 1
    io = VgxTimelinesChain()
    io.popNum, io.hapNum, io.susNum, io.ev_ptr = m.popNum, m.hapNum, m.susNum, int(ev.ptr)
    io.ev_times, io.ev_types, io.ev_haplotypes = _p(ev.times), _p(ev.types), _p(ev.haplotypes)
    io.ev_populations, io.ev_newHaplotypes, io.ev_newPopulations = _p(ev.populations), _p(ev.newHaplotypes), _p(ev.newPopulations)
    io.currentTime, io.step_num, io.semantics = float(m.currentTime), int(step_num), TIMELINE_SEMANTICS[semantics]

    def start(q, table, width):
        ok = (q[:, 0] >= 0) & (q[:, 0] < m.popNum) & (q[:, 1] >= 0) & (q[:, 1] < width)   # (the library refuses the others)
        out = np.zeros(len(q), dtype=np.int64)
        out[ok] = np.asarray(table, dtype=np.int64)[q[ok, 0], q[ok, 1]]
        return out
    keep = [np.ascontiguousarray(qi[:, 0]), np.ascontiguousarray(qi[:, 1]), start(qi, m.initial_infectious, m.hapNum),
            np.ascontiguousarray(qs[:, 0]), np.ascontiguousarray(qs[:, 1]), start(qs, m.initial_susceptible, m.susNum)]
    io.n_inf, io.inf_pop, io.inf_hap, io.inf_start = len(qi), _p(keep[0]), _p(keep[1]), _p(keep[2])
    io.n_sus, io.sus_pop, io.sus_grp, io.sus_start = len(qs), _p(keep[3]), _p(keep[4]), _p(keep[5])
    tp = np.zeros(T)
    inf, smp, sus = np.zeros((max(len(qi), 1), T)), np.zeros((max(len(qi), 1), T)), np.zeros((max(len(qs), 1), T))
    io.time_points, io.inf_data, io.inf_sample, io.sus_data = _p(tp), _p(inf), _p(smp), _p(sus)

    def finish(chain=io, _alive=keep):   # (the query arrays live as long as this closure)
        return {"time_points": tp, "infectious": inf[:len(qi)][ii], "samples": smp[:len(qi)][ii], "susceptible": sus[:len(qs)][si],
                "last_point": int(chain.last_point)}
    return io, finish


def replay_timelines(m, infectious=(), susceptible=(), step_num=100, semantics='reference'):
    """The log replays of ``Ensemble.timelines`` for one host model through ``vgx_test_timelines``: the device replay's code
    (vgx_tline.h) compiled for the host, on ``m.events``, ``m.currentTime`` and ``m.initial_*`` (direct chains only; no GPU).
    Returns a dict: ``time_points`` [T], ``infectious`` / ``samples`` [Ki, T], ``susceptible`` [Ks, T], ``last_point``."""
    io, finish = _timelines_chain(m, infectious, susceptible, step_num, semantics)
    err = C.create_string_buffer(512)
    if load_library().vgx_test_timelines(C.byref(io), err, 512) != 0:
        raise ValueError(err.value.decode() or "vgx_test_timelines failed")
    return finish()


MEV_COLUMNS = ("num", "types", "haplotypes", "populations", "newHaplotypes", "newPopulations")


def replay_tau_timelines(m, infectious=(), susceptible=(), step_num=100, semantics='reference', mev=None):
    """The log replays of ``Ensemble.tau_timelines`` for one host model through ``vgx_test_tau_timelines``: the device replay's
    code (weighted rows, flattening, cut search; vgx_tline.h, vgx_tau_timelines.hip) compiled for the host, on ``m.events`` with
    the multievent rows its MULTITYPE events index (no GPU).  ``mev``: a dict of the columns num, types, haplotypes, populations,
    newHaplotypes, newPopulations (dense logs with ``num == 0`` rows are fine); default ``m.multievents``.  Same dict as
    ``replay_timelines``."""
    io, finish = _timelines_chain(m, infectious, susceptible, step_num, semantics)
    tio = VgxTauTimelinesChain()
    tio.chain = io
    if mev is None:
        mv = m.multievents
        mev = {c: getattr(mv, c)[:mv.ptr] for c in MEV_COLUMNS}
    cols = [np.ascontiguousarray(mev[c], dtype=np.int64) for c in MEV_COLUMNS]
    if len({len(c) for c in cols}) != 1:
        raise ValueError("multievent columns of different lengths")
    tio.mev_rows = len(cols[0])
    for name, col in zip(MEV_COLUMNS, cols):
        setattr(tio, "mev_" + name, _p(col))
    err = C.create_string_buffer(512)
    if load_library().vgx_test_tau_timelines(C.byref(tio), err, 512) != 0:
        raise ValueError(err.value.decode() or "vgx_test_tau_timelines failed")
    return finish(tio.chain)


def haplotype_mask(haplotypes, hapNum):
    """The bitmask ``vgx_get_incidence`` takes for a haplotype filter: bit h of word h // 32 for every index in ``haplotypes``
    (uint32, ceil(hapNum / 32) words); ValueError for an index outside [0, hapNum)."""
    idx = np.asarray(haplotypes).ravel()
    if len(idx) and not np.issubdtype(idx.dtype, np.integer):
        raise ValueError("haplotypes must be integer indices")
    idx = idx.astype(np.int64)
    if len(idx) and (idx.min() < 0 or idx.max() >= hapNum):
        raise ValueError("haplotype index out of range")
    mask = np.zeros((int(hapNum) + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(mask, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)).astype(np.uint32))
    return mask


def replay_incidence(times, types, haplotypes, populations, newHaplotypes, newPopulations, popNum, hapNum, edges, hap_mask=None, tile=0):
    """The event counts of ``Ensemble.incidence`` for one chain given as arrays through ``vgx_test_incidence``: the device's rule
    and tile walk (vgx_incidence.h) compiled for the host, tile after tile of ``tile`` events (0: the default); no GPU.
    ``hap_mask``: None or the words of ``haplotype_mask``.  Returns (counts [T, P, 7] int32, outside [2] int64); a refusal raises
    ``ValueError`` with the library's message."""
    times = np.ascontiguousarray(times, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.int64) for c in (types, haplotypes, populations, newHaplotypes, newPopulations)]
    n = len(times)
    if any(len(c) != n for c in cols):
        raise ValueError("event columns of different lengths")
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    T = len(edges) - 1
    counts = np.zeros((max(T, 1), max(int(popNum), 1), len(INCIDENCE_CHANNELS)), dtype=np.int32)
    outside = np.zeros(2, dtype=np.int64)
    mask = None if hap_mask is None else np.ascontiguousarray(hap_mask, dtype=np.uint32)
    if mask is not None and len(mask) != (int(hapNum) + 31) // 32:
        raise ValueError("hap_mask must hold ceil(hapNum / 32) words")
    err = C.create_string_buffer(512)
    rc = load_library().vgx_test_incidence(_p(times), *[_p(c) for c in cols], n, int(popNum), int(hapNum), _p(edges), T,
                                           None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint32)), int(tile),
                                           counts.ctypes.data_as(C.POINTER(C.c_int32)), _p(outside), err, 512)
    if rc != VGX_OK:
        raise ValueError(err.value.decode() or "vgx_test_incidence failed")
    return counts, outside


def variant_map(variants, hapNum):
    """The map ``vgx_get_prevalence`` takes, (variant_of [hapNum] int32 with values in [-1, V), V), from what ``Ensemble.prevalence``
    accepts as ``variants``: None (every haplotype its own class, V = hapNum); an integer array [hapNum] with values -1 (not
    tracked) or a class (V = the largest class + 1, at least 1); or a sequence of sequences of haplotype indices (class k = the k-th
    sequence, unlisted haplotypes not tracked).  ValueError for anything else."""
    H = int(hapNum)
    if variants is None:
        return np.arange(H, dtype=np.int32), H
    if len(variants) and all(np.ndim(v) == 1 for v in variants):   # classes as lists of haplotypes
        vo = np.full(H, -1, dtype=np.int32)
        for k, members in enumerate(variants):
            idx = np.asarray(members).ravel()
            if len(idx) and not np.issubdtype(idx.dtype, np.integer):
                raise ValueError("variants must hold integer haplotype indices")
            idx = idx.astype(np.int64)
            if len(idx) and (idx.min() < 0 or idx.max() >= H):
                raise ValueError("haplotype index out of range")
            if len(np.unique(idx)) != len(idx) or (vo[idx] >= 0).any():
                raise ValueError("a haplotype is listed twice in variants")
            vo[idx] = k
        return vo, len(variants)
    a = np.asarray(variants)
    if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("variants must be an integer array [hapNum] or a sequence of sequences of haplotype indices")
    if len(a) != H:
        raise ValueError("variants must hold one class per haplotype (%d), got %d" % (H, len(a)))
    V = max(int(a.max()) + 1, 1)
    if a.min() < -1 or V > np.iinfo(np.int32).max:
        raise ValueError("variant_of[%d] = %d is outside [-1, %d)" % (int(a.argmin()), int(a.min()), V))
    return np.ascontiguousarray(a, dtype=np.int32), V


def replay_prevalence(times, types, haplotypes, populations, newHaplotypes, newPopulations, popNum, hapNum, grid, variant_of, V, start, tile=0):
    """The values of ``Ensemble.prevalence`` for one chain given as arrays through ``vgx_test_prevalence``: the device's rule, tile
    walk and scan (vgx_prevalence.h) compiled for the host, tile after tile of ``tile`` events (0: the default); no GPU.
    ``variant_of`` [hapNum] with values in [-1, V); ``start`` [P, V] the chain's start folded through it.  Returns (values
    [T, P, V] int32, final [P, V] int32, outside [2] int64); a refusal raises ``ValueError`` with the library's message."""
    times = np.ascontiguousarray(times, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.int64) for c in (types, haplotypes, populations, newHaplotypes, newPopulations)]
    n = len(times)
    if any(len(c) != n for c in cols):
        raise ValueError("event columns of different lengths")
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    T, P, V = len(grid), int(popNum), int(V)
    vo = np.ascontiguousarray(variant_of, dtype=np.int32)
    if len(vo) != int(hapNum):
        raise ValueError("variant_of must hold hapNum values")
    start = np.ascontiguousarray(start, dtype=np.int64)
    if start.shape != (P, V):
        raise ValueError("start must have the shape [P, V]")
    values = np.zeros((max(T, 1), max(P, 1), max(V, 1)), dtype=np.int32)
    final = np.zeros((max(P, 1), max(V, 1)), dtype=np.int32)
    outside = np.zeros(2, dtype=np.int64)
    err = C.create_string_buffer(512)
    i32 = C.POINTER(C.c_int32)
    rc = load_library().vgx_test_prevalence(_p(times), *[_p(c) for c in cols], n, P, int(hapNum), _p(grid), T, vo.ctypes.data_as(i32), V,
                                            _p(start), int(tile), values.ctypes.data_as(i32), final.ctypes.data_as(i32), _p(outside), err, 512)
    if rc != VGX_OK:
        raise ValueError(err.value.decode() or "vgx_test_prevalence failed")
    return values, final, outside


def replay_lineages(m, seed, grid, variant_of, V, tile=0, rng_raw=None):
    """The values of ``Ensemble.lineages`` for the chain and state of one host model through ``vgx_test_lineages``: the device's walk
    with its observer, tile walk and suffix sum (vgx_gwalk.h, vgx_lineages.h) compiled for the host, tile after tile of ``tile``
    lineage records (0: the default); no GPU.  ``seed`` and ``rng_raw`` as ``get_genealogy`` takes them (a direct chain;
    ``seed=None`` without ``rng_raw`` starts at the simulation stream's origin); ``variant_of`` [hapNum] with values in [-1, V).
    Walks ``m.infectious`` back in place.  Returns a dict: values [T, P, V] int32, root [P, V] int32, records, nodes_used,
    rng_raw; a refusal or a walk that fails raises ``ValueError`` with the library's message."""
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    T, P, V = len(grid), int(m.popNum), int(V)
    vo = np.ascontiguousarray(variant_of, dtype=np.int32)
    if len(vo) != int(m.hapNum):
        raise ValueError("variant_of must hold hapNum values")
    io, _, _ = _genealogy_chain(m, seed, None, rng_raw)
    values = np.zeros((max(T, 1), max(P, 1), max(V, 1)), dtype=np.int32)
    root = np.zeros((max(P, 1), max(V, 1)), dtype=np.int32)
    records = np.zeros(1, dtype=np.int64)
    err = C.create_string_buffer(512)
    i32 = C.POINTER(C.c_int32)
    rc = load_library().vgx_test_lineages(C.byref(io), _p(grid), T, vo.ctypes.data_as(i32), V, int(tile), values.ctypes.data_as(i32),
                                          root.ctypes.data_as(i32), _p(records), err, 512)
    if rc != VGX_OK:
        raise ValueError(err.value.decode() or "vgx_test_lineages failed")
    return {"values": values, "root": root, "records": int(records[0]), "nodes_used": int(io.nodes_used),
            "rng_raw": tuple(int(io.rng_state[i]) for i in range(4)) + (0, 0)}


def replay_tau_lineages(m, seed, grid, variant_of, V, tile=0, rng_position=None, rng_raw=None):
    """The values of ``Ensemble.tau_lineages`` for the chain and state of one host model through ``vgx_test_tau_lineages``: the tau
    walk of the device pass with its observer, the tile walk and the suffix sum (vgx_gwalk_tau.h, vgx_lineages.h) compiled for
    the host, tile after tile of ``tile`` lineage records (0: the default); no GPU.  The chain as ``tau_genealogy_walk`` takes it
    (its trailing MULTITYPE events play a replicate's own steps, rows in any order and granularity); ``seed``, ``rng_position``
    and ``rng_raw`` as ``get_genealogy``; ``variant_of`` [hapNum] with values in [-1, V).  Walks ``m.infectious`` back in place.
    Returns the dict of ``replay_lineages`` with all six words in ``rng_raw``; a refusal or a walk that fails raises
    ``ValueError`` with the library's message (a failed walk: the text ``tau_genealogy_walk`` raises)."""
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    T, P, V = len(grid), int(m.popNum), int(V)
    vo = np.ascontiguousarray(variant_of, dtype=np.int32)
    if len(vo) != int(m.hapNum):
        raise ValueError("variant_of must hold hapNum values")
    io, _, _ = _genealogy_chain(m, seed, rng_position, rng_raw)
    values = np.zeros((max(T, 1), max(P, 1), max(V, 1)), dtype=np.int32)
    root = np.zeros((max(P, 1), max(V, 1)), dtype=np.int32)
    records = np.zeros(1, dtype=np.int64)
    err = C.create_string_buffer(512)
    i32 = C.POINTER(C.c_int32)
    rc = load_library().vgx_test_tau_lineages(C.byref(io), int(m.sites), _p(grid), T, vo.ctypes.data_as(i32), V, int(tile),
                                              values.ctypes.data_as(i32), root.ctypes.data_as(i32), _p(records), err, 512)
    if rc != VGX_OK:
        raise ValueError(err.value.decode() or "vgx_test_tau_lineages failed")
    return {"values": values, "root": root, "records": int(records[0]), "nodes_used": int(io.nodes_used),
            "rng_raw": tuple(int(io.rng_state[i]) for i in range(4)) + (int(io.rng_has_uint32), int(io.rng_uinteger))}


def replay_tree_events(m, seed, grid, variant_of, V, tile=0, rng_position=None, rng_raw=None, tau=False):
    """The block of ``Ensemble.tree_events`` (``tau=True``: ``Ensemble.tau_tree_events``) for the chain and state of one host model
    through ``vgx_test_tree_events`` (``vgx_test_tau_tree_events``): the walk of ``replay_lineages`` (``replay_tau_lineages``) with
    the host tile walk of vgx_tree_events.h, tile after tile of ``tile`` lineage records (0: the default); no GPU.  Arguments as
    those take them.  Walks ``m.infectious`` back in place.  Returns a dict: counts [T + 1, P, V, 7] int32, records, nodes_used,
    rng_raw; a refusal or a walk that fails raises ``ValueError`` with the library's message."""
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    T, P, V = len(grid), int(m.popNum), int(V)
    vo = np.ascontiguousarray(variant_of, dtype=np.int32)
    if len(vo) != int(m.hapNum):
        raise ValueError("variant_of must hold hapNum values")
    io, _, _ = _genealogy_chain(m, seed, rng_position if tau else None, rng_raw)
    counts = np.zeros((T + 1, max(P, 1), max(V, 1), len(TREE_EVENT_CHANNELS)), dtype=np.int32)
    records = np.zeros(1, dtype=np.int64)
    err = C.create_string_buffer(512)
    i32 = C.POINTER(C.c_int32)
    tail = (_p(grid), T, vo.ctypes.data_as(i32), V, int(tile), counts.ctypes.data_as(i32), _p(records), err, 512)
    if tau:
        rc = load_library().vgx_test_tau_tree_events(C.byref(io), int(m.sites), *tail)
    else:
        rc = load_library().vgx_test_tree_events(C.byref(io), *tail)
    if rc != VGX_OK:
        raise ValueError(err.value.decode() or "vgx_test_tree_events failed")
    return {"counts": counts, "records": int(records[0]), "nodes_used": int(io.nodes_used),
            "rng_raw": tuple(int(io.rng_state[i]) for i in range(4)) + ((int(io.rng_has_uint32), int(io.rng_uinteger)) if tau else (0, 0))}


FLOW_FORMS = {None: 0, 'auto': 0, 'dense': 1, 'split': 2}   # VGX_FLOW_AUTO, VGX_FLOW_DENSE, VGX_FLOW_SPLIT
FLOW_FORM_NAMES = {0: None, 1: 'dense', 2: 'split'}


def _tree_arrays(tree, node_ev, times):
    i32 = C.POINTER(C.c_int32)
    t = np.ascontiguousarray(tree, dtype=np.int64).ravel()
    ev = np.ascontiguousarray(node_ev, dtype=np.int64).ravel()
    tm = np.ascontiguousarray(times, dtype=np.float64).ravel()
    if not (len(t) == len(ev) == len(tm)):
        raise ValueError("tree, node_ev and times must have one entry per node")
    for name, a in (("tree", t), ("node_ev", ev)):
        if len(a) and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise ValueError("%s does not fit 32 bits" % name)
    t, ev = t.astype(np.int32), ev.astype(np.int32)
    return t, ev, tm, i32


def tree_shape(tree, node_ev, times):
    """The row of ``Ensemble.tree_shapes`` for one tree through ``vgx_test_tree_shape``: the sequential sweep of vgx_tree_shape.h on
    the host; no GPU.  ``tree`` parents (-1 at the last node, the root), ``node_ev`` event indices, ``times`` node times, one entry per
    node.  Returns (stats int64 [12], lengths float64 [7]) in the order of ``TREE_SHAPE_STATS`` and ``TREE_SHAPE_LENGTHS``; raises
    ``ValueError`` naming the first offending node for a tree that is not binary in creation order."""
    t, ev, tm, i32 = _tree_arrays(tree, node_ev, times)
    stats, lengths = np.zeros(len(TREE_SHAPE_STATS), dtype=np.int64), np.zeros(len(TREE_SHAPE_LENGTHS), dtype=np.float64)
    err = C.create_string_buffer(512)
    rc = load_library().vgx_test_tree_shape(t.ctypes.data_as(i32), ev.ctypes.data_as(i32), _p(tm), len(t), _p(stats), _p(lengths), err, 512)
    if rc != VGX_OK:
        raise ValueError(err.value.decode() or "vgx_test_tree_shape failed")
    return stats, lengths


def tree_shape_device(trees):
    """The rows of given trees through the kernel of ``Ensemble.tree_shapes`` (``vgx_test_tree_shape_device``, one launch, no engine).
    ``trees``: a sequence of (tree, node_ev, times) as ``tree_shape`` takes them.  Returns (stats [n, 12], lengths [n, 7], status
    [n, 2]: status and its argument, ``GW_BAD_TREE`` and the node for a tree with a node of one child or more than two; its row holds
    zeros and NaN).  Parents outside the tree are refused with ``ValueError`` before anything is uploaded."""
    parts = [_tree_arrays(*tr)[:3] for tr in trees]
    n = len(parts)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(p[0]) for p in parts])
    i32 = C.POINTER(C.c_int32)
    t = np.ascontiguousarray(np.concatenate([p[0] for p in parts]) if n else np.zeros(0, np.int32), dtype=np.int32)
    ev = np.ascontiguousarray(np.concatenate([p[1] for p in parts]) if n else np.zeros(0, np.int32), dtype=np.int32)
    tm = np.ascontiguousarray(np.concatenate([p[2] for p in parts]) if n else np.zeros(0), dtype=np.float64)
    stats = np.zeros((max(n, 1), len(TREE_SHAPE_STATS)), dtype=np.int64)
    lengths = np.zeros((max(n, 1), len(TREE_SHAPE_LENGTHS)), dtype=np.float64)
    status = np.zeros((max(n, 1), 2), dtype=np.int64)
    err = C.create_string_buffer(512)
    rc = load_library().vgx_test_tree_shape_device(n, _p(off), t.ctypes.data_as(i32), ev.ctypes.data_as(i32), _p(tm), _p(stats), _p(lengths),
                                                   _p(status), err, 512)
    if rc == 1:
        raise ValueError(err.value.decode())
    if rc != VGX_OK:
        raise VgxError(rc, err.value.decode() or "vgx_test_tree_shape_device failed")
    return stats[:n], lengths[:n], status[:n]


def _spectrum_arrays(tree, mut_node, mut_AS, mut_DS, mut_site):
    t = np.ascontiguousarray(tree, dtype=np.int64).ravel()
    cols = [np.ascontiguousarray(c, dtype=np.int64).ravel() for c in (mut_node, mut_AS, mut_DS, mut_site)]
    if len({len(c) for c in cols}) != 1:
        raise ValueError("mut_node, mut_AS, mut_DS and mut_site must have one entry per record")
    for name, a in zip(("tree", "mut_node", "mut_AS", "mut_DS", "mut_site"), [t] + cols):
        if len(a) and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise ValueError("%s does not fit 32 bits" % name)
    return [t.astype(np.int32)] + [c.astype(np.int32) for c in cols]


def mutation_spectrum(tree, mut_node, mut_AS, mut_DS, mut_site, sites, with_clade=False):
    """The row of ``Ensemble.mutation_spectrum`` for one tree through ``vgx_test_mutation_spectrum``: the sequential sweep of
    vgx_mutation_spectrum.h (the definition) on the host; no GPU.  ``tree`` parents (-1 at the last node, the root), one entry per
    node; the four record columns, one entry per mutation record; ``sites`` the model's sites (0 .. 15).  Returns (spectrum int64
    [sites, 32], substitutions [sites, 4, 4], sums [sites, 3], stats [4]) in the order of ``MUTATION_SPECTRUM_SUMS`` and
    ``MUTATION_SPECTRUM_STATS``, with ``clade`` int32 [nodes] appended when ``with_clade``; raises ``ValueError`` naming the node of a
    tree that is not binary in creation order, or the record that lies outside the tree or the model."""
    t, mn, mA, mD, ms = _spectrum_arrays(tree, mut_node, mut_AS, mut_DS, mut_site)
    S, i32 = int(sites), C.POINTER(C.c_int32)
    if not 0 <= S <= 15:
        raise ValueError("sites = %d (0 .. 15)" % S)
    spectrum, subs = np.zeros((S, MUTATION_SPECTRUM_BINS), dtype=np.int64), np.zeros((S, 4, 4), dtype=np.int64)
    sums, stats = np.zeros((S, len(MUTATION_SPECTRUM_SUMS)), dtype=np.int64), np.zeros(len(MUTATION_SPECTRUM_STATS), dtype=np.int64)
    clade = np.zeros(max(len(t), 1), dtype=np.int32)
    err = C.create_string_buffer(512)
    rc = load_library().vgx_test_mutation_spectrum(t.ctypes.data_as(i32), len(t), mn.ctypes.data_as(i32), mA.ctypes.data_as(i32),
                                                   mD.ctypes.data_as(i32), ms.ctypes.data_as(i32), len(mn), S, _p(spectrum), _p(subs), _p(sums),
                                                   _p(stats), clade.ctypes.data_as(i32), err, 512)
    if rc != VGX_OK:
        raise ValueError(err.value.decode() or "vgx_test_mutation_spectrum failed")
    return (spectrum, subs, sums, stats) + ((clade[:len(t)],) if with_clade else ())


def mutation_spectrum_device(trees, sites, walk_status=None):
    """The rows of given trees through the kernel of ``Ensemble.mutation_spectrum`` (``vgx_test_mutation_spectrum_device``, one launch,
    no engine).  ``trees``: a sequence of (tree, mut_node, mut_AS, mut_DS, mut_site) as ``mutation_spectrum`` takes them; ``sites`` is
    shared.  ``walk_status``: None, or [n, 2] a walk status and its argument per tree (a tree whose status is not 0 is skipped).
    Returns (spectrum [n, sites, 32], substitutions [n, sites, 4, 4], sums [n, sites, 3], stats [n, 4], status [n, 2], clade: a list
    of int32 arrays, one per tree).  ``status`` is 0, the given walk status, ``GW_BAD_TREE`` and the node, or ``GW_BAD_RECORD`` and the
    lowest offending record; the last three come with an all-zero row.  Parents outside the tree are refused with ``ValueError``
    before anything is uploaded; a bad record does reach the device."""
    parts = [_spectrum_arrays(*tr) for tr in trees]
    n, S, i32 = len(parts), int(sites), C.POINTER(C.c_int32)
    if not 0 <= S <= 15:
        raise ValueError("sites = %d (0 .. 15)" % S)
    node_off, mut_off = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    node_off[1:] = np.cumsum([len(p[0]) for p in parts])
    mut_off[1:] = np.cumsum([len(p[1]) for p in parts])
    cat = [np.ascontiguousarray(np.concatenate([p[k] for p in parts] + [np.zeros(1, np.int32)]), dtype=np.int32) for k in range(5)]
    ws = None
    if walk_status is not None:
        ws = np.ascontiguousarray(walk_status, dtype=np.int64).reshape(n, 2)
    spectrum, subs = np.zeros((max(n, 1), S, MUTATION_SPECTRUM_BINS), dtype=np.int64), np.zeros((max(n, 1), S, 4, 4), dtype=np.int64)
    sums = np.zeros((max(n, 1), S, len(MUTATION_SPECTRUM_SUMS)), dtype=np.int64)
    stats, status = np.zeros((max(n, 1), len(MUTATION_SPECTRUM_STATS)), dtype=np.int64), np.zeros((max(n, 1), 2), dtype=np.int64)
    clade = np.zeros(int(node_off[n]) + 1, dtype=np.int32)
    err = C.create_string_buffer(512)
    rc = load_library().vgx_test_mutation_spectrum_device(n, _p(node_off), cat[0].ctypes.data_as(i32), _p(mut_off), cat[1].ctypes.data_as(i32),
                                                          cat[2].ctypes.data_as(i32), cat[3].ctypes.data_as(i32), cat[4].ctypes.data_as(i32), S,
                                                          _p(ws) if ws is not None else None, _p(spectrum), _p(subs), _p(sums), _p(stats),
                                                          _p(status), clade.ctypes.data_as(i32), err, 512)
    if rc == 1:
        raise ValueError(err.value.decode())
    if rc != VGX_OK:
        raise VgxError(rc, err.value.decode() or "vgx_test_mutation_spectrum_device failed")
    return (spectrum[:n], subs[:n], sums[:n], stats[:n], status[:n],
            [clade[node_off[t]:node_off[t + 1]].copy() for t in range(n)])


def _labelled_tree(tree, pop):
    t, p = np.ascontiguousarray(tree, dtype=np.int64).ravel(), np.ascontiguousarray(pop, dtype=np.int64).ravel()
    if len(t) != len(p):
        raise ValueError("tree and pop must have one entry per node")
    for name, a in (("tree", t), ("pop", p)):
        if len(a) and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise ValueError("%s does not fit 32 bits" % name)
    return t.astype(np.int32), p.astype(np.int32)


def _introductions_blocks(n, P):
    return (np.zeros((n, P), dtype=np.int64), np.zeros((n, P, P), dtype=np.int64), np.zeros((n, P, len(INTRODUCTIONS_INTO)), dtype=np.int64),
            np.zeros((n, P, INTRODUCTIONS_BINS), dtype=np.int64), np.zeros((n, len(INTRODUCTIONS_STATS)), dtype=np.int64))


def introductions(tree, pop, pops, with_nodes=False):
    """The row of ``Ensemble.introductions`` for one tree through ``vgx_test_introductions``: the sequential sweep of
    vgx_introductions.h (the definition) on the host; no GPU.  ``tree`` parents (-1 at the last node, the root) and ``pop`` the
    population label, one entry per node; ``pops`` the model's populations (1 .. 1024).  Returns (tips_by_pop int64 [pops], imports
    [pops, pops] by (source, destination), into [pops, 6], spectrum [pops, 32], stats [8]) in the order of ``INTRODUCTIONS_INTO`` and
    ``INTRODUCTIONS_STATS``, with ``clade`` and ``local`` int32 [nodes] appended when ``with_nodes``; raises ``ValueError`` naming the
    node of a tree that is not binary in creation order, or the node whose label lies outside the model."""
    t, p = _labelled_tree(tree, pop)
    P, i32 = int(pops), C.POINTER(C.c_int32)
    if not 1 <= P <= INTRODUCTIONS_POPS_MAX:
        raise ValueError("populations = %d (1 .. %d)" % (P, INTRODUCTIONS_POPS_MAX))
    blocks = [b[0] for b in _introductions_blocks(1, P)]
    clade, local = np.zeros(max(len(t), 1), dtype=np.int32), np.zeros(max(len(t), 1), dtype=np.int32)
    err = C.create_string_buffer(512)
    rc = load_library().vgx_test_introductions(t.ctypes.data_as(i32), p.ctypes.data_as(i32), len(t), P, *[_p(b) for b in blocks],
                                               clade.ctypes.data_as(i32), local.ctypes.data_as(i32), err, 512)
    if rc != VGX_OK:
        raise ValueError(err.value.decode() or "vgx_test_introductions failed")
    return tuple(blocks) + ((clade[:len(t)], local[:len(t)]) if with_nodes else ())


def introductions_device(trees, pops, walk_status=None):
    """The rows of given trees through the kernel of ``Ensemble.introductions`` (``vgx_test_introductions_device``, one launch, no
    engine).  ``trees``: a sequence of (tree, pop) as ``introductions`` takes them; ``pops`` is shared.  ``walk_status``: None, or
    [n, 2] a walk status and its argument per tree (a tree whose status is not 0 is skipped).  Returns (tips_by_pop [n, pops],
    imports [n, pops, pops], into [n, pops, 6], spectrum [n, pops, 32], stats [n, 8], status [n, 2]).  ``status`` is 0, the given
    walk status, ``GW_BAD_TREE`` and the node, or ``GW_BAD_LABEL`` and the lowest offending node; the last three come with an
    all-zero row.  Parents outside the tree are refused with ``ValueError`` before anything is uploaded; a bad label does reach the
    device."""
    parts = [_labelled_tree(*tr) for tr in trees]
    n, P, i32 = len(parts), int(pops), C.POINTER(C.c_int32)
    if not 1 <= P <= INTRODUCTIONS_POPS_MAX:
        raise ValueError("populations = %d (1 .. %d)" % (P, INTRODUCTIONS_POPS_MAX))
    node_off = np.zeros(n + 1, dtype=np.int64)
    node_off[1:] = np.cumsum([len(p[0]) for p in parts])
    cat = [np.ascontiguousarray(np.concatenate([p[k] for p in parts] + [np.zeros(1, np.int32)]), dtype=np.int32) for k in range(2)]
    ws = None
    if walk_status is not None:
        ws = np.ascontiguousarray(walk_status, dtype=np.int64).reshape(n, 2)
    blocks = _introductions_blocks(max(n, 1), P)
    status = np.zeros((max(n, 1), 2), dtype=np.int64)
    err = C.create_string_buffer(512)
    rc = load_library().vgx_test_introductions_device(n, _p(node_off), cat[0].ctypes.data_as(i32), cat[1].ctypes.data_as(i32), P,
                                                      _p(ws) if ws is not None else None, *[_p(b) for b in blocks], _p(status), err, 512)
    if rc == 1:
        raise ValueError(err.value.decode())
    if rc != VGX_OK:
        raise VgxError(rc, err.value.decode() or "vgx_test_introductions_device failed")
    return tuple(b[:n] for b in blocks) + (status[:n],)


def _event_indices(node_ev):
    ev = np.ascontiguousarray(node_ev, dtype=np.int64).ravel()
    if len(ev) and (ev.min() < -2 ** 31 or ev.max() >= 2 ** 31):
        raise ValueError("node_ev does not fit 32 bits")
    return ev.astype(np.int32)


def tau_node_times(node_ev, pre_times, step_times):
    """The node times of one tree of a tau chain through ``vgx_test_tau_node_times``: the rule of vgx_tau_tree_shape.h on the host; no
    GPU.  ``node_ev`` the nodes' event indices in a chain of ``len(pre_times)`` prefix events followed by ``len(step_times)`` own
    steps.  Returns float64 [nodes]: 0.0 for a negative index, the prefix event's or the step's time otherwise; raises ``ValueError``
    naming the node for an index beyond the chain."""
    ev = _event_indices(node_ev)
    pre = np.ascontiguousarray(pre_times, dtype=np.float64).ravel()
    st = np.ascontiguousarray(step_times, dtype=np.float64).ravel()
    times = np.zeros(len(ev), dtype=np.float64)
    err = C.create_string_buffer(512)
    rc = load_library().vgx_test_tau_node_times(ev.ctypes.data_as(C.POINTER(C.c_int32)), len(ev), len(pre), _p(pre), len(st), _p(st), _p(times),
                                                err, 512)
    if rc != VGX_OK:
        raise ValueError(err.value.decode() or "vgx_test_tau_node_times failed")
    return times


def tau_node_times_device(trees, pre_times):
    """The node times of given trees through the node-time kernel of ``Ensemble.tau_tree_shapes`` (``vgx_test_tau_node_times_device``,
    one launch, no engine).  ``trees``: a sequence of (node_ev, n_pre, step_times): the tree's event indices, how many events of the
    shared table ``pre_times`` its chain starts with (0: a replicate that restarted) and its own step times.  Returns (a list of
    float64 arrays, one per tree, and bad int32 [n]: the lowest node whose index lies beyond its chain, whose time is 0.0, or
    ``INT32_MAX``).  An index beyond the chain does reach the device: the kernel checks every index before it loads."""
    pre = np.ascontiguousarray(pre_times, dtype=np.float64).ravel()
    evs = [_event_indices(t[0]) for t in trees]
    sts = [np.ascontiguousarray(t[2], dtype=np.float64).ravel() for t in trees]
    n = len(evs)
    node_off, step_off = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    node_off[1:], step_off[1:] = np.cumsum([len(x) for x in evs]), np.cumsum([len(x) for x in sts])
    n_pre = np.ascontiguousarray([int(t[1]) for t in trees] + [0], dtype=np.int64)
    ev = np.ascontiguousarray(np.concatenate(evs + [np.zeros(1, np.int32)]), dtype=np.int32)
    st = np.ascontiguousarray(np.concatenate(sts + [np.zeros(1)]), dtype=np.float64)
    times = np.zeros(len(ev), dtype=np.float64)
    bad = np.zeros(n + 1, dtype=np.int32)
    i32 = C.POINTER(C.c_int32)
    err = C.create_string_buffer(512)
    rc = load_library().vgx_test_tau_node_times_device(n, _p(node_off), ev.ctypes.data_as(i32), _p(n_pre), len(pre), _p(pre), _p(step_off), _p(st),
                                                       _p(times), bad.ctypes.data_as(i32), err, 512)
    if rc == 1:
        raise ValueError(err.value.decode())
    if rc != VGX_OK:
        raise VgxError(rc, err.value.decode() or "vgx_test_tau_node_times_device failed")
    return [times[node_off[t]:node_off[t + 1]].copy() for t in range(n)], bad[:n]


def replay_flows(times, types, haplotypes, populations, newHaplotypes, newPopulations, popNum, hapNum, edges, variant_of, V, within=True,
                 tile=0, form=None):
    """The block of ``Ensemble.flows`` for one chain given as arrays through ``vgx_test_flows``: the device's rule and tile walk
    (vgx_flows.h) compiled for the host, tile after tile of ``tile`` events (0: the default), in the form ``form`` asks for
    (None: the automatic choice, 'dense', 'split'); no GPU.  ``variant_of`` [hapNum] with values in [-1, V).  Returns (counts
    [T, P, P, V] int32 in src, dst, class order, outside [2] int64, the form that ran); a refusal raises ``ValueError`` with the
    library's message."""
    times = np.ascontiguousarray(times, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.int64) for c in (types, haplotypes, populations, newHaplotypes, newPopulations)]
    n = len(times)
    if any(len(c) != n for c in cols):
        raise ValueError("event columns of different lengths")
    if form not in FLOW_FORMS:
        raise ValueError("form must be None, 'dense' or 'split'")
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    T, P, V = len(edges) - 1, int(popNum), int(V)
    vo = np.ascontiguousarray(variant_of, dtype=np.int32)
    if len(vo) != int(hapNum):
        raise ValueError("variant_of must hold hapNum values")
    counts = np.zeros((max(T, 1), max(P, 1), max(P, 1), max(V, 1)), dtype=np.int32)
    outside = np.zeros(2, dtype=np.int64)
    ran = np.zeros(1, dtype=np.int64)
    err = C.create_string_buffer(512)
    i32 = C.POINTER(C.c_int32)
    rc = load_library().vgx_test_flows(_p(times), *[_p(c) for c in cols], n, P, int(hapNum), _p(edges), T, vo.ctypes.data_as(i32), V,
                                       1 if within else 0, int(tile), FLOW_FORMS[form], counts.ctypes.data_as(i32), _p(outside), _p(ran), err, 512)
    if rc != VGX_OK:
        raise ValueError(err.value.decode() or "vgx_test_flows failed")
    return counts, outside, FLOW_FORM_NAMES[int(ran[0])]


MS_NEVER = 2 ** 31 - 1     # VGX_MS_NEVER: first_event of a threshold no value reaches
MS_MAX_K = 16


def milestone_thresholds(thresholds):
    """``thresholds`` of ``Ensemble.milestones`` as an int32 array [K], K <= 16; ValueError for anything else."""
    th = np.asarray(thresholds if thresholds is not None else ())
    if th.ndim != 1:
        raise ValueError("thresholds must be a sequence of integers")
    if len(th) and not np.issubdtype(th.dtype, np.integer):
        raise ValueError("thresholds must be integers")
    if len(th) > MS_MAX_K:
        raise ValueError("K = %d thresholds: at most %d" % (len(th), MS_MAX_K))
    th = th.astype(object) if len(th) else th
    if len(th) and (min(th) < -2 ** 31 or max(th) > 2 ** 31 - 1):
        raise ValueError("thresholds must be integers in int32")
    return np.ascontiguousarray(th, dtype=np.int32)


def milestones_lds_check(P, V, K):
    """The LDS limit of the walk, worded as the library words it; ValueError above it."""
    need = (P + 1) * V * 4 * (4 + K)
    if need > 65536:
        raise ValueError("%d populations (and their total) x %d classes x %d thresholds need %d bytes of records, above the 65536 bytes of "
                         "LDS a walking workgroup may use" % (P, V, K, need))


def replay_milestones(times, types, haplotypes, populations, newHaplotypes, newPopulations, popNum, hapNum, variant_of, V, start, thresholds=(),
                      tile=0, t_start=0.0):
    """The results of ``Ensemble.milestones`` for one chain given as arrays through ``vgx_test_milestones``: the device's rule, tile
    bases, rounds of 64 lanes and merge (vgx_milestones.h) compiled for the host, tile after tile of ``tile`` events (0: the
    default); no GPU.  ``variant_of`` [hapNum] with values in [-1, V); ``start`` [P, V] the chain's start folded through it;
    ``t_start`` the time of event index -1.  Returns a dict of final, peak, peak_event, last_positive_event [P + 1, V] int32,
    first_event [K, P + 1, V] int32, peak_time, extinction_time [P + 1, V] and first_time [K, P + 1, V] float64; a refusal raises
    ``ValueError`` with the library's message."""
    times = np.ascontiguousarray(times, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.int64) for c in (types, haplotypes, populations, newHaplotypes, newPopulations)]
    n = len(times)
    if any(len(c) != n for c in cols):
        raise ValueError("event columns of different lengths")
    P, V = int(popNum), int(V)
    vo = np.ascontiguousarray(variant_of, dtype=np.int32)
    if len(vo) != int(hapNum):
        raise ValueError("variant_of must hold hapNum values")
    start = np.ascontiguousarray(start, dtype=np.int64)
    if start.shape != (P, V):
        raise ValueError("start must have the shape [P, V]")
    th = np.ascontiguousarray(thresholds, dtype=np.int32).ravel()
    K = len(th)
    shape, kshape = (P + 1, max(V, 1)), (max(K, 1), P + 1, max(V, 1))
    out = {k: np.zeros(shape, dtype=np.int32) for k in ("final", "peak", "peak_event", "last_positive_event")}
    out["first_event"] = np.zeros(kshape, dtype=np.int32)
    out["peak_time"], out["extinction_time"] = np.zeros(shape), np.zeros(shape)
    out["first_time"] = np.zeros(kshape)
    err = C.create_string_buffer(512)
    i32 = C.POINTER(C.c_int32)
    rc = load_library().vgx_test_milestones(
        _p(times), *[_p(c) for c in cols], n, P, int(hapNum), vo.ctypes.data_as(i32), V, _p(start), th.ctypes.data_as(i32), K, int(tile),
        float(t_start), *[out[k].ctypes.data_as(i32) for k in ("final", "peak", "peak_event", "last_positive_event", "first_event")],
        *[_p(out[k]) for k in ("peak_time", "extinction_time", "first_time")], err, 512)
    if rc != VGX_OK:
        raise ValueError(err.value.decode() or "vgx_test_milestones failed")
    for k in ("first_event", "first_time"):
        out[k] = out[k][:K]
    return out


def tau_milestone_thresholds(thresholds):
    """``thresholds`` of ``Ensemble.tau_milestones`` as an int64 array [K], K <= 16; ValueError for anything else."""
    th = np.asarray(thresholds if thresholds is not None else ())
    if th.ndim != 1:
        raise ValueError("thresholds must be a sequence of integers")
    if len(th) and th.dtype != object and not np.issubdtype(th.dtype, np.integer):
        raise ValueError("thresholds must be integers")
    if len(th) > MS_MAX_K:
        raise ValueError("K = %d thresholds: at most %d" % (len(th), MS_MAX_K))
    th = th.astype(object) if len(th) else th
    if len(th) and not all(isinstance(t, (int, np.integer)) and not isinstance(t, bool) for t in th):
        raise ValueError("thresholds must be integers")
    if len(th) and (min(th) < -2 ** 63 or max(th) > 2 ** 63 - 1):
        raise ValueError("thresholds must be integers in int64")
    return np.ascontiguousarray(th, dtype=np.int64)


def tau_milestones_lds_check(P, V, K):
    """The LDS limit of the tau walk (vgx_tau_ms_lds_bytes), worded as the library words it; ValueError above it."""
    need = (P + 1) * V * (40 + 4 * K) + 16
    if need > 65536:
        raise ValueError("%d populations (and their total) x %d classes x %d thresholds need %d bytes of records, above the 65536 bytes of "
                         "LDS a walking workgroup may use" % (P, V, K, need))


def replay_tau_milestones(events, mev, popNum, hapNum, variant_of, V, start, thresholds=(), tile=0, n_own_events=-1, t_start=0.0):
    """The results of ``Ensemble.tau_milestones`` for one chain through ``vgx_test_tau_milestones``: the device's flattening, tile
    edges, tile bases, settle, merge in tile order and outputs (vgx_tau_milestones.h) compiled for the host, tile after tile of about
    ``tile`` rows (0: the default); no GPU.  ``events`` and ``mev`` as ``replay_tau_incidence`` takes them; the last ``n_own_events``
    events play the replicate's own steps (-1: the trailing MULTITYPE events), everything before them the prefix, which is walked
    once as a chain of its own.  ``variant_of`` [hapNum] with values in [-1, V); ``start`` [P, V] the chain's start folded through
    it; ``thresholds`` int64; ``t_start`` the time of event index -1.  Returns a dict of final, peak [P + 1, V] int64, peak_event,
    last_positive_event [P + 1, V] int32, first_event [K, P + 1, V] int32, peak_time, extinction_time [P + 1, V] and first_time
    [K, P + 1, V] float64; a refusal raises ``ValueError`` with the library's message."""
    times = np.ascontiguousarray(events[0], dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.int64) for c in events[1:6]]
    n = len(times)
    if len(cols) != 5 or any(len(c) != n for c in cols):
        raise ValueError("event columns of different lengths")
    mcols = [np.ascontiguousarray(mev[c] if mev is not None else [], dtype=np.int64) for c in MEV_COLUMNS]
    if len({len(c) for c in mcols}) != 1:
        raise ValueError("multievent columns of different lengths")
    P, V = int(popNum), int(V)
    vo = np.ascontiguousarray(variant_of, dtype=np.int32)
    if len(vo) != int(hapNum):
        raise ValueError("variant_of must hold hapNum values")
    start = np.ascontiguousarray(start, dtype=np.int64)
    if start.shape != (P, V):
        raise ValueError("start must have the shape [P, V]")
    th = np.ascontiguousarray(thresholds, dtype=np.int64).ravel()
    K = len(th)
    shape, kshape = (P + 1, max(V, 1)), (max(K, 1), P + 1, max(V, 1))
    out = {k: np.zeros(shape, dtype=np.int64) for k in ("final", "peak")}
    out.update({k: np.zeros(shape, dtype=np.int32) for k in ("peak_event", "last_positive_event")})
    out["first_event"] = np.zeros(kshape, dtype=np.int32)
    out["peak_time"], out["extinction_time"] = np.zeros(shape), np.zeros(shape)
    out["first_time"] = np.zeros(kshape)
    i32 = C.POINTER(C.c_int32)
    io = VgxTauMilestonesChain()
    io.popNum, io.hapNum, io.ev_ptr, io.ev_times = P, int(hapNum), n, _p(times)
    for name, col in zip(("types", "haplotypes", "populations", "newHaplotypes", "newPopulations"), cols):
        setattr(io, "ev_" + name, _p(col))
    io.mev_rows = len(mcols[0])
    for name, col in zip(MEV_COLUMNS, mcols):
        setattr(io, "mev_" + name, _p(col))
    io.V, io.variant_of, io.start, io.K, io.thresholds = V, vo.ctypes.data_as(i32), _p(start), K, _p(th)
    io.tile, io.n_own_events, io.t_start = int(tile), int(n_own_events), float(t_start)
    io.final, io.peak = _p(out["final"]), _p(out["peak"])
    for k in ("peak_event", "last_positive_event", "first_event"):
        setattr(io, k, out[k].ctypes.data_as(i32))
    for k in ("peak_time", "extinction_time", "first_time"):
        setattr(io, k, _p(out[k]))
    err = C.create_string_buffer(512)
    if load_library().vgx_test_tau_milestones(C.byref(io), err, 512) != VGX_OK:
        raise ValueError(err.value.decode() or "vgx_test_tau_milestones failed")
    for k in ("first_event", "first_time"):
        out[k] = out[k][:K]
    return out


def replay_tau_incidence(events, mev, popNum, hapNum, edges, hap_mask=None, tile=0, n_own_events=-1):
    """The event counts of ``Ensemble.tau_incidence`` for one chain through ``vgx_test_tau_incidence``: the device's flattening,
    cuts, cells and tile walk (vgx_tau_incidence.h) compiled for the host, tile after tile of ``tile`` rows (0: the default); no GPU.
    ``events``: the six event columns (times, types, haplotypes, populations, newHaplotypes, newPopulations); ``mev``: a dict of the
    multievent columns num, types, haplotypes, populations, newHaplotypes, newPopulations that the MULTITYPE events index, or None.
    The last ``n_own_events`` events play the replicate's own steps (-1: the trailing MULTITYPE events), everything before them the
    prefix, which is counted once and added as on the device.  ``hap_mask``: None or the words of ``haplotype_mask``.  Returns
    (counts [T, P, 7] int64, outside [2] int64); a refusal raises ``ValueError`` with the library's message."""
    times = np.ascontiguousarray(events[0], dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.int64) for c in events[1:6]]
    n = len(times)
    if len(cols) != 5 or any(len(c) != n for c in cols):
        raise ValueError("event columns of different lengths")
    mcols = [np.ascontiguousarray(mev[c] if mev is not None else [], dtype=np.int64) for c in MEV_COLUMNS]
    if len({len(c) for c in mcols}) != 1:
        raise ValueError("multievent columns of different lengths")
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    T = len(edges) - 1
    counts = np.zeros((max(T, 1), max(int(popNum), 1), len(INCIDENCE_CHANNELS)), dtype=np.int64)
    outside = np.zeros(2, dtype=np.int64)
    mask = None if hap_mask is None else np.ascontiguousarray(hap_mask, dtype=np.uint32)
    if mask is not None and len(mask) != (int(hapNum) + 31) // 32:
        raise ValueError("hap_mask must hold ceil(hapNum / 32) words")
    io = VgxTauIncidenceChain()
    io.popNum, io.hapNum, io.ev_ptr, io.ev_times = int(popNum), int(hapNum), n, _p(times)
    for name, col in zip(("types", "haplotypes", "populations", "newHaplotypes", "newPopulations"), cols):
        setattr(io, "ev_" + name, _p(col))
    io.mev_rows = len(mcols[0])
    for name, col in zip(MEV_COLUMNS, mcols):
        setattr(io, "mev_" + name, _p(col))
    io.T, io.edges = T, _p(edges)
    io.hap_mask = None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint32))
    io.tile, io.n_own_events = int(tile), int(n_own_events)
    io.counts, io.outside = _p(counts), _p(outside)
    err = C.create_string_buffer(512)
    if load_library().vgx_test_tau_incidence(C.byref(io), err, 512) != VGX_OK:
        raise ValueError(err.value.decode() or "vgx_test_tau_incidence failed")
    return counts, outside


def tau_flows_lds_check(P, V):
    """The LDS limit of the split form of ``vgx_get_tau_flows`` (8-byte cells), worded as the library words it; ValueError above it."""
    need = 8 * P * V
    if need > 65536:
        raise ValueError("%d populations x %d classes need %d bytes of 8-byte cells in the split form, above the 65536 bytes of LDS a "
                         "counting workgroup may use" % (P, V, need))


def replay_tau_flows(events, mev, P, H, edges, variant_of, V, within=True, tile=0, form=0, n_own=-1):
    """The block of ``Ensemble.tau_flows`` for one chain through ``vgx_test_tau_flows``: the device's flattening, cuts, cell and
    tile walk (vgx_tau_flows.h) compiled for the host, tile after tile of ``tile`` rows (0: the default), in the form ``form`` asks
    for (0 or None: the automatic choice, 1 or 'dense', 2 or 'split'); no GPU.  ``events`` and ``mev`` as ``replay_tau_incidence``
    takes them; the last ``n_own`` events play the replicate's own steps (-1: the trailing MULTITYPE events), everything before them
    the prefix, which is counted once and added as on the device.  ``variant_of`` [H] with values in [-1, V).  Returns (counts
    [T, P, P, V] int64 in src, dst, class order, outside [2] int64, the form that ran: 'dense' or 'split'); a refusal raises
    ``ValueError`` with the library's message."""
    times = np.ascontiguousarray(events[0], dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.int64) for c in events[1:6]]
    n = len(times)
    if len(cols) != 5 or any(len(c) != n for c in cols):
        raise ValueError("event columns of different lengths")
    mcols = [np.ascontiguousarray(mev[c] if mev is not None else [], dtype=np.int64) for c in MEV_COLUMNS]
    if len({len(c) for c in mcols}) != 1:
        raise ValueError("multievent columns of different lengths")
    if form is None or isinstance(form, str):
        if form not in FLOW_FORMS:
            raise ValueError("form must be None, 'dense' or 'split'")
        form = FLOW_FORMS[form]
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    T, P, H, V = len(edges) - 1, int(P), int(H), int(V)
    vo = np.ascontiguousarray(variant_of, dtype=np.int32)
    if len(vo) != H:
        raise ValueError("variant_of must hold hapNum values")
    fits = 0 < P and 0 < V and 8 * P * V <= 65536   # (what does not fit is refused by the hook before it writes)
    counts = np.zeros((max(T, 1), P, P, V) if fits else (1,), dtype=np.int64)
    outside = np.zeros(2, dtype=np.int64)
    io = VgxTauFlowsChain()
    io.popNum, io.hapNum, io.ev_ptr, io.ev_times = P, H, n, _p(times)
    for name, col in zip(("types", "haplotypes", "populations", "newHaplotypes", "newPopulations"), cols):
        setattr(io, "ev_" + name, _p(col))
    io.mev_rows = len(mcols[0])
    for name, col in zip(MEV_COLUMNS, mcols):
        setattr(io, "mev_" + name, _p(col))
    io.T, io.edges, io.V, io.variant_of = T, _p(edges), V, vo.ctypes.data_as(C.POINTER(C.c_int32))
    io.within, io.tile, io.form, io.n_own_events = 1 if within else 0, int(tile), int(form), int(n_own)
    io.counts, io.outside = _p(counts), _p(outside)
    err = C.create_string_buffer(512)
    if load_library().vgx_test_tau_flows(C.byref(io), err, 512) != VGX_OK:
        raise ValueError(err.value.decode() or "vgx_test_tau_flows failed")
    return counts, outside, FLOW_FORM_NAMES[int(io.form_ran)]


def replay_tau_prevalence(events, mev, popNum, hapNum, grid, variant_of, V, start, tile=0, n_own_events=-1):
    """The values of ``Ensemble.tau_prevalence`` for one chain through ``vgx_test_tau_prevalence``: the device's flattening, bounds,
    signed cells, tile walk, prefix-plus-own sum and scan (vgx_tau_prevalence.h) compiled for the host, tile after tile of ``tile``
    rows (0: the default); no GPU.  ``events`` and ``mev`` as ``replay_tau_incidence`` takes them; the last ``n_own_events`` events
    play the replicate's own steps (-1: the trailing MULTITYPE events), everything before them the prefix, which is counted once
    as on the device.  ``variant_of`` [hapNum] with values in [-1, V); ``start`` [P, V] the chain's start folded through it.
    Returns (values [T, P, V] int64, final [P, V] int64, outside [2] int64); a refusal raises ``ValueError`` with the library's
    message."""
    times = np.ascontiguousarray(events[0], dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.int64) for c in events[1:6]]
    n = len(times)
    if len(cols) != 5 or any(len(c) != n for c in cols):
        raise ValueError("event columns of different lengths")
    mcols = [np.ascontiguousarray(mev[c] if mev is not None else [], dtype=np.int64) for c in MEV_COLUMNS]
    if len({len(c) for c in mcols}) != 1:
        raise ValueError("multievent columns of different lengths")
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    T, P, V = len(grid), int(popNum), int(V)
    vo = np.ascontiguousarray(variant_of, dtype=np.int32)
    if len(vo) != int(hapNum):
        raise ValueError("variant_of must hold hapNum values")
    start = np.ascontiguousarray(start, dtype=np.int64)
    if start.shape != (P, V):
        raise ValueError("start must have the shape [P, V]")
    values = np.zeros((max(T, 1), max(P, 1), max(V, 1)), dtype=np.int64)
    final = np.zeros((max(P, 1), max(V, 1)), dtype=np.int64)
    outside = np.zeros(2, dtype=np.int64)
    io = VgxTauPrevalenceChain()
    io.popNum, io.hapNum, io.ev_ptr, io.ev_times = P, int(hapNum), n, _p(times)
    for name, col in zip(("types", "haplotypes", "populations", "newHaplotypes", "newPopulations"), cols):
        setattr(io, "ev_" + name, _p(col))
    io.mev_rows = len(mcols[0])
    for name, col in zip(MEV_COLUMNS, mcols):
        setattr(io, "mev_" + name, _p(col))
    io.T, io.grid, io.V, io.variant_of, io.start = T, _p(grid), V, vo.ctypes.data_as(C.POINTER(C.c_int32)), _p(start)
    io.tile, io.n_own_events = int(tile), int(n_own_events)
    io.values, io.final, io.outside = _p(values), _p(final), _p(outside)
    err = C.create_string_buffer(512)
    if load_library().vgx_test_tau_prevalence(C.byref(io), err, 512) != VGX_OK:
        raise ValueError(err.value.decode() or "vgx_test_tau_prevalence failed")
    return values, final, outside


def group_map(groups, susNum):
    """The map ``vgx_get_susceptibles`` takes, (class_of [susNum] int32 with values in [-1, G), G), from what
    ``Ensemble.susceptibles`` accepts as ``groups``: what ``variant_map`` does, over the susceptibility groups.  None (every group
    its own class, G = susNum); an integer array [susNum] with values -1 (not tracked) or a class (G = the largest class + 1, at
    least 1); or a sequence of sequences of group indices (class k = the k-th sequence, unlisted groups not tracked).  ValueError
    for anything else."""
    S = int(susNum)
    if groups is None:
        return np.arange(S, dtype=np.int32), S
    if len(groups) and all(np.ndim(v) == 1 for v in groups):   # classes as lists of groups
        co = np.full(S, -1, dtype=np.int32)
        for k, members in enumerate(groups):
            idx = np.asarray(members).ravel()
            if len(idx) and not np.issubdtype(idx.dtype, np.integer):
                raise ValueError("groups must hold integer susceptibility group indices")
            idx = idx.astype(np.int64)
            if len(idx) and (idx.min() < 0 or idx.max() >= S):
                raise ValueError("susceptibility group index out of range")
            if len(np.unique(idx)) != len(idx) or (co[idx] >= 0).any():
                raise ValueError("a susceptibility group is listed twice in groups")
            co[idx] = k
        return co, len(groups)
    a = np.asarray(groups)
    if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("groups must be an integer array [susNum] or a sequence of sequences of group indices")
    if len(a) != S:
        raise ValueError("groups must hold one class per susceptibility group (%d), got %d" % (S, len(a)))
    G = max(int(a.max()) + 1, 1)
    if a.min() < -1 or G > np.iinfo(np.int32).max:
        raise ValueError("class_of[%d] = %d is outside [-1, %d)" % (int(a.argmin()), int(a.min()), G))
    return np.ascontiguousarray(a, dtype=np.int32), G


def replay_susceptibles(times, types, haplotypes, populations, newHaplotypes, newPopulations, popNum, susNum, grid, class_of, G, start, tile=0):
    """The values of ``Ensemble.susceptibles`` for one chain given as arrays through ``vgx_test_susceptibles``: the device's rule
    (vgx_susceptible.h), tile walk and scan compiled for the host, tile after tile of ``tile`` events (0: the default); no GPU.
    ``class_of`` [susNum] with values in [-1, G); ``start`` [P, G] the chain's susceptible start folded through it.  Returns
    (values [T, P, G] int32, final [P, G] int32, outside [2] int64); a refusal raises ``ValueError`` with the library's message."""
    times = np.ascontiguousarray(times, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.int64) for c in (types, haplotypes, populations, newHaplotypes, newPopulations)]
    n = len(times)
    if any(len(c) != n for c in cols):
        raise ValueError("event columns of different lengths")
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    T, P, G = len(grid), int(popNum), int(G)
    co = np.ascontiguousarray(class_of, dtype=np.int32)
    if len(co) != int(susNum):
        raise ValueError("class_of must hold susNum values")
    start = np.ascontiguousarray(start, dtype=np.int64)
    if start.shape != (P, G):
        raise ValueError("start must have the shape [P, G]")
    values = np.zeros((max(T, 1), max(P, 1), max(G, 1)), dtype=np.int32)
    final = np.zeros((max(P, 1), max(G, 1)), dtype=np.int32)
    outside = np.zeros(2, dtype=np.int64)
    err = C.create_string_buffer(512)
    i32 = C.POINTER(C.c_int32)
    rc = load_library().vgx_test_susceptibles(_p(times), *[_p(c) for c in cols], n, P, int(susNum), _p(grid), T, co.ctypes.data_as(i32), G,
                                              _p(start), int(tile), values.ctypes.data_as(i32), final.ctypes.data_as(i32), _p(outside), err, 512)
    if rc != VGX_OK:
        raise ValueError(err.value.decode() or "vgx_test_susceptibles failed")
    return values, final, outside


def replay_tau_susceptibles(events, mev, popNum, susNum, grid, class_of, G, start, tile=0, n_own_events=-1):
    """The values of ``Ensemble.tau_susceptibles`` for one chain through ``vgx_test_tau_susceptibles``: ``replay_tau_prevalence``
    over the susceptible rule (vgx_tau_susceptible.h); no GPU.  ``events``, ``mev`` and ``n_own_events`` as there; ``class_of``
    [susNum] with values in [-1, G); ``start`` [P, G].  Returns (values [T, P, G] int64, final [P, G] int64, outside [2] int64); a
    refusal raises ``ValueError`` with the library's message."""
    times = np.ascontiguousarray(events[0], dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.int64) for c in events[1:6]]
    n = len(times)
    if len(cols) != 5 or any(len(c) != n for c in cols):
        raise ValueError("event columns of different lengths")
    mcols = [np.ascontiguousarray(mev[c] if mev is not None else [], dtype=np.int64) for c in MEV_COLUMNS]
    if len({len(c) for c in mcols}) != 1:
        raise ValueError("multievent columns of different lengths")
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    T, P, G = len(grid), int(popNum), int(G)
    co = np.ascontiguousarray(class_of, dtype=np.int32)
    if len(co) != int(susNum):
        raise ValueError("class_of must hold susNum values")
    start = np.ascontiguousarray(start, dtype=np.int64)
    if start.shape != (P, G):
        raise ValueError("start must have the shape [P, G]")
    values = np.zeros((max(T, 1), max(P, 1), max(G, 1)), dtype=np.int64)
    final = np.zeros((max(P, 1), max(G, 1)), dtype=np.int64)
    outside = np.zeros(2, dtype=np.int64)
    io = VgxTauSusceptiblesChain()
    io.popNum, io.susNum, io.ev_ptr, io.ev_times = P, int(susNum), n, _p(times)
    for name, col in zip(("types", "haplotypes", "populations", "newHaplotypes", "newPopulations"), cols):
        setattr(io, "ev_" + name, _p(col))
    io.mev_rows = len(mcols[0])
    for name, col in zip(MEV_COLUMNS, mcols):
        setattr(io, "mev_" + name, _p(col))
    io.T, io.grid, io.G, io.class_of, io.start = T, _p(grid), G, co.ctypes.data_as(C.POINTER(C.c_int32)), _p(start)
    io.tile, io.n_own_events = int(tile), int(n_own_events)
    io.values, io.final, io.outside = _p(values), _p(final), _p(outside)
    err = C.create_string_buffer(512)
    if load_library().vgx_test_tau_susceptibles(C.byref(io), err, 512) != VGX_OK:
        raise ValueError(err.value.decode() or "vgx_test_tau_susceptibles failed")
    return values, final, outside


def column_summary(x, group_of, G, ranks):
    """The kernels of ``vgx_get_trajectory_summary`` on a host matrix ``x`` [R, N] of whole numbers in [0, 2^31) through
    ``vgx_test_column_summary``: ``group_of`` [R] in [-1, G), ``ranks`` [G, K].  Returns a dict: ``count`` [G], ``sum``, ``min``,
    ``max`` [G, N] int64, ``sumsq`` [G, N, 2] uint64 (low, high word), ``stat`` [G, K, N] int64, ``passes``, ``ms``.  A refusal
    raises ``VgxError`` with the library's message."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    R, N = x.shape
    group_of = np.ascontiguousarray(group_of, dtype=np.int64)
    ranks = np.ascontiguousarray(ranks, dtype=np.int64).reshape(G, -1)
    assert group_of.shape == (R,)
    K = ranks.shape[1]
    out = {k: np.zeros((G, N), dtype=np.int64) for k in ("sum", "min", "max")}
    out["count"] = np.zeros(G, dtype=np.int64)
    out["stat"] = np.zeros((G, max(K, 1), N), dtype=np.int64)
    sumsq = np.zeros((G, N, 2), dtype=np.uint64)
    io = VgxTrajSummaryIO()
    io.G, io.group_of, io.K, io.ranks = G, _p(group_of), K, _p(ranks)
    for k, a in out.items():
        setattr(io, k, _p(a))
    io.sumsq = sumsq.ctypes.data_as(C.POINTER(C.c_uint64))
    err = C.create_string_buffer(512)
    rc = load_library().vgx_test_column_summary(_p(x), R, N, C.byref(io), err, 512)
    if rc != VGX_OK:
        raise VgxError(rc, err.value.decode())
    out["stat"] = out["stat"][:, :K]
    out["sumsq"], out["passes"], out["ms"] = sumsq, int(io.passes), tuple(io.ms)
    return out


def direct_plan(shape, mode=0, kernel=0):
    """The kernel choice of a direct call through ``vgx_test_direct_plan``: ``shape`` maps the fields of ``vgx_direct_shape`` to
    integers (missing ones are 0).  Returns the fields of ``vgx_direct_plan`` as a dict; a refused request raises ``VgxError``
    with the library's message."""
    lib = load_library()
    s, o, plan = VgxDirectShape(**{k: int(v) for k, v in shape.items()}), VgxRunOpts(), VgxDirectPlan()
    o.record_events, o.mode, o.kernel = 1, int(mode), int(kernel)
    err = C.create_string_buffer(1024)
    rc = lib.vgx_test_direct_plan(C.byref(s), C.byref(o), C.byref(plan), err, 1024)
    if rc != 0:
        raise VgxError(rc, err.value.decode())
    return {name: int(getattr(plan, name)) for name, _ in VgxDirectPlan._fields_}


def propensity_scan(infectious, rates123, numToHap, bRate, susceptibility, rowSusceptible, rowContact, u, bench_rows=0, repeats=3):
    """The dense propensity row pass (``vgx_propensity_scan``, K3): returns a dict of the output arrays.  With ``bench_rows``
    the first row is replicated that many times in HBM and timed (``ms_update``, ``ms_choose`` in the result)."""
    lib = load_library()
    inf = np.ascontiguousarray(infectious, dtype=np.int64)
    rows, H = inf.shape
    S = int(np.asarray(susceptibility).reshape(H, -1).shape[1])
    n = bench_rows if bench_rows else rows

    def fit(a, shape):   # bench mode: per-row inputs are given per synthetic row, or repeated
        a = np.ascontiguousarray(a, dtype=np.float64).reshape((-1,) + shape)
        return np.ascontiguousarray(np.resize(a, (n,) + shape)) if len(a) != n else a
    keep = dict(infectious=inf, eventRates123=np.ascontiguousarray(rates123, dtype=np.float64).reshape(rows, H, 3),
                numToHap=np.ascontiguousarray(numToHap, dtype=np.int64), bRate=np.ascontiguousarray(bRate, dtype=np.float64),
                susceptibility=np.ascontiguousarray(susceptibility, dtype=np.float64).reshape(H, S),
                rowSusceptible=fit(rowSusceptible, (S,)), rowContact=fit(rowContact, ()), u=fit(u, ()))
    ro = 1 if bench_rows else rows
    out = dict(birthRate=np.zeros((ro, H)), tEvent=np.zeros((ro, H)), hapPopRate=np.zeros((ro, H)),
               susceptHapPopRate=np.zeros((ro, H, S)), rowTotal=np.zeros(ro), chosen=np.zeros(ro, dtype=np.int64), rnOut=np.zeros(ro))
    io = VgxRowScan()
    io.rows, io.H, io.S = rows, H, S
    for k, v in list(keep.items()) + list(out.items()):
        setattr(io, k, _p(v))
    if bench_rows:
        a, b = C.c_double(0), C.c_double(0)
        rc = lib.vgx_propensity_scan_bench(C.byref(io), int(bench_rows), int(repeats), C.byref(a), C.byref(b))
        out["ms_update"], out["ms_choose"] = a.value, b.value
    else:
        rc = lib.vgx_propensity_scan(C.byref(io))
    if rc != VGX_OK:
        raise VgxError(rc, lib.vgx_propensity_scan_error().decode())
    return out
