// The device code of the fit path (abn_api.hip includes this, and it alone; the three kernels only the plan launches are
// abn_plan_kernels.hpp's, for abn_plan.hip; the pairwise scans of abn_pairwise.hip, the window placement of abn_windows.hip
// and the analysis of abn_analyze.hip have headers of their own).
#pragma once
#include "abn_common.hpp"
#include "abn_fit_kernel.hpp"
#include "abn_fit_refill.hpp"
#include "abn_fit_spec.hpp"
#include "abn_fit_sweep.hpp"
#include "abn_aux_kernels.hpp"
