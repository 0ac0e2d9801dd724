"""The public surface of the binding, pinned: the package's public module-level names and, for every public class, its
public members with the signature of each method.  The table is the package as it was when the binding was one module
(its incidental imports `Path` and `annotations` left out); a name that moves to another module stays importable from
the package, with the signature it had."""
import inspect


def surface(pkg):
    """(public non-module names; {class: {public member or __init__: str(signature) of a method, None of anything else}},
    the members being those the package's own classes define, inherited ones included)"""
    names, classes = [], {}
    for name, v in sorted(vars(pkg).items()):
        if name.startswith("_") or inspect.ismodule(v):
            continue
        names.append(name)
        if inspect.isclass(v):
            own = [k for k in v.__mro__ if k.__module__.startswith(pkg.__name__)]
            members = {}
            for m in sorted({m for k in own for m in vars(k) if m == "__init__" or not m.startswith("_")}):
                f = inspect.getattr_static(v, m)
                f = f.__func__ if isinstance(f, (classmethod, staticmethod)) else f
                members[m] = str(inspect.signature(f)) if inspect.isfunction(f) else None
            classes[name] = members
    return names, classes


NAMES = ['ABN_OK', 'AbnError', 'CONTEXTS', 'Codes', 'Context', 'EXPORTED_SYMBOLS', 'FIT_CONVERGED', 'FIT_INFO_DTYPE',
 'FIT_MAX_ITERS', 'FIT_NONFINITE', 'FIT_TARGET', 'GeneRule', 'Genes', 'KERNEL_NAMES', 'LIB_PATH', 'MultiPlan',
 'Options', 'PKG', 'Plan', 'STATUS_NAMES', 'Sites', 'SitesParams', 'Tiles', 'Windows', 'WindowsParams', 'analyze',
 'analyze_batch', 'block_counts_host', 'block_resample_host', 'default_options', 'device_count', 'gen_boot_simplices',
 'gen_start_simplices', 'load_host_library', 'load_library', 'multi_plan_shard', 'pack_codes', 'packed_row_stride',
 'rccl_available', 'reduction_tree', 'sort_sites_host', 'unpack_codes']
CLASSES = {'AbnError': {'__init__': "(self, status: 'int', detail: 'str' = '')"},
 'Codes': {'close': '(self)',
           'common': '(self)',
           'from_parsed': "(cls, ctx: 'Context', sites_list, *, posterior_max_filter, align=False)",
           'info': '(self)',
           'kernel_ms': "(self) -> 'np.ndarray'",
           'packed': "(self) -> 'np.ndarray'",
           'packed_device_ptr': "(self) -> 'int'",
           'pairwise': '(self)',
           'stats': '(self)',
           'transitions': '(self)',
           'union': '(self)'},
 'Context': {'__init__': "(self, device: 'int' = 0, stream: 'int | None' = None)",
             'ab_neutral_run': "(self, pedigree, p0uu, eqp, eqp_weight, n_starts, *, options: 'Options | None' = None)",
             'analyze_batch_dev': "(self, raw_ptr: 'int', n_windows: 'int', n_boot: 'int', out_ptr: 'int', "
                                  "first_bad_ptr: 'int' = 0, allow_failed_windows=False) -> 'float'",
             'block_counts': "(self, seed: 'int', group_id, group_begin, group_end, n_replicates: 'int', n_blocks: "
                             "'int') -> 'np.ndarray'",
             'block_resample': '(self, group_begin, group_end, counts, both, diff, level_sum_kept, kept)',
             'block_resample_dev': "(self, group_begin, group_end, rows_per_group: 'int', counts_ptr: 'int', n_blocks: "
                                   "'int', n_pairs: 'int', n_samples: 'int', both_ptr: 'int', diff_ptr: 'int', "
                                   "level_ptr: 'int', kept_ptr: 'int', both_out_ptr: 'int' = 0, diff_out_ptr: 'int' = "
                                   "0, dvalue_out_ptr: 'int' = 0, level_out_ptr: 'int' = 0, kept_out_ptr: 'int' = 0) "
                                   "-> 'np.ndarray'",
             'boot_model_run': '(self, pedigree, model, pred, resid, p0uu, eqp, eqp_weight, n_boot, *, options: '
                               "'Options | None' = None)",
             'bootstrap_rows': '(self, best)',
             'choose_genes': '(self, genes: "\'Genes\'", site_offset, chromosome, start, end, strand, *, cutoff, '
                             'cutoff_gene_length=False)',
             'choose_genes_dev': '(self, genes: "\'Genes\'", site_offset, chromosome_ptr: \'int\', start_ptr: \'int\', '
                                 "end_ptr: 'int', strand_ptr: 'int', gene_start_ptr: 'int', gene_end_ptr: 'int', "
                                 "flags_ptr: 'int', *, cutoff, cutoff_gene_length=False) -> 'np.ndarray'",
             'close': '(self)',
             'common_sites': '(self, site_offset, chromosome, start, end, strand)',
             'cost_batch': '(self, pedigree, p_uu0, eqp, eqp_weight, candidates, *, pred=None, resid=None, idx=None, '
                           "cand_to_boot=None, options: 'Options | None' = None, want_dt=False, want_puu=False)",
             'device_info': '(self)',
             'fit_batch': '(self, pedigree, p_uu0, eqp, eqp_weight, simplex0, max_iters, *, dobs_rows=None, options: '
                          "'Options | None' = None)",
             'fit_batch_sweep': '(self, pedigree, p_uu0, eqp, eqp_weight, simplex0, max_iters, *, dobs_rows=None, '
                                "options: 'Options | None' = None)",
             'gen_boot_indices': "(self, seed, window, b0, nb, n_rows) -> 'np.ndarray'",
             'pairwise_divergence': '(self, codes)',
             'pairwise_divergence_dev': "(self, codes_ptr: 'int', n_samples: 'int', n_sites: 'int', diff_ptr: 'int' = "
                                        "0, both_ptr: 'int' = 0, dvalue_ptr: 'int' = 0) -> 'float'",
             'pairwise_divergence_packed': "(self, packed, n_sites: 'int')",
             'pairwise_divergence_packed_dev': "(self, packed_ptr: 'int', n_samples: 'int', n_sites: 'int', "
                                               "row_stride: 'int', diff_ptr: 'int' = 0, both_ptr: 'int' = 0, "
                                               "dvalue_ptr: 'int' = 0) -> 'float'",
             'pairwise_divergence_windows': '(self, codes, begin, end)',
             'pairwise_divergence_windows_dev': "(self, codes_ptr: 'int', n_samples: 'int', row_stride: 'int', begin, "
                                                "end, diff_ptr: 'int' = 0, both_ptr: 'int' = 0, dvalue_ptr: 'int' = 0) "
                                                "-> 'float'",
             'pairwise_divergence_windows_packed': "(self, packed, n_sites: 'int', begin, end)",
             'pairwise_divergence_windows_packed_dev': "(self, packed_ptr: 'int', n_samples: 'int', n_sites: 'int', "
                                                       "row_stride: 'int', begin, end, diff_ptr: 'int' = 0, both_ptr: "
                                                       "'int' = 0, dvalue_ptr: 'int' = 0) -> 'float'",
             'pairwise_transitions_packed': "(self, packed, n_sites: 'int')",
             'pairwise_transitions_packed_dev': "(self, packed_ptr: 'int', n_samples: 'int', n_sites: 'int', "
                                                "row_stride: 'int', table_ptr: 'int') -> 'float'",
             'pairwise_transitions_windows_packed': "(self, packed, n_sites: 'int', begin, end)",
             'pairwise_transitions_windows_packed_dev': "(self, packed_ptr: 'int', n_samples: 'int', n_sites: 'int', "
                                                        "row_stride: 'int', begin, end, table_ptr: 'int') -> 'float'",
             'parse_sites': "(self, text: 'bytes', *, skip_lines: 'int' = 1, slab_bytes: 'int' = 0, contexts=('CG',))",
             'parse_sites_resident': "(self, text: 'bytes', *, skip_lines: 'int' = 1, slab_bytes: 'int' = 0, "
                                     'contexts=(\'CG\',)) -> "\'Sites\'"',
             'select_best': '(self, pedigree, p0uu, models)',
             'sort_sites': '(self, chromosome, start, end, strand)',
             'union_sites': '(self, site_offset, chromosome, start, end, strand)'},
 'GeneRule': {'cutoff': None, 'cutoff_gene_length': None},
 'Genes': {'__init__': '(self, ctx: "\'Context\'", lists)', 'close': '(self)'},
 'MultiPlan': {'__init__': "(self, devices, generations, n_windows, n_starts, n_boot, *, options: 'Options | None' = "
                           'None)',
               'analyze': '(self, allow_failed_windows=False)',
               'close': '(self)',
               'counters': '(self)',
               'download': '(self, want_info=True, allow_failed_windows=False)',
               'kernel_ms': "(self, device_index: 'int' = 0)",
               'run': '(self)',
               'set_stream_sweep': "(self, mode: 'int')",
               'set_window_ids': '(self, ids)',
               'set_windows': '(self, d_obs, p0uu, eqp=None, eqp_weight=None)',
               'shard': "(self, device_index: 'int')",
               'sync': '(self)'},
 'Options': {'lanes_per_chain': None,
             'max_iters_boot': None,
             'max_iters_start': None,
             'no_fixed_point_skip': None,
             'sd_tolerance': None,
             'seed': None,
             'shrink_on_failed_contraction': None,
             'stream_mode': None,
             'strict_order': None,
             'window_groups': None},
 'Plan': {'__init__': "(self, ctx: 'Context', generations, n_windows, n_starts, n_boot, *, window_offset=0, "
                      "boot_offset=0, options: 'Options | None' = None)",
          'analyze': '(self, allow_failed_windows=False)',
          'bind_raw': "(self, dev_ptr: 'int')",
          'close': '(self)',
          'counters': '(self)',
          'device_bytes': "(self) -> 'int'",
          'download': '(self, want_info=True, allow_failed_windows=False)',
          'early_bootstraps': '(self)',
          'failed_windows': "(self) -> 'int'",
          'kernel_ms': '(self)',
          'last_kernels': '(self)',
          'raw_device_ptr': "(self) -> 'int'",
          'run': '(self)',
          'run_phase': "(self, phase: 'int')",
          'set_early_bootstraps': "(self, mode: 'int')",
          'set_stream_sweep': "(self, mode: 'int')",
          'set_window_ids': '(self, ids)',
          'set_windows': '(self, d_obs, p0uu, eqp=None, eqp_weight=None)',
          'stream_sweep': '(self)',
          'sync': '(self)',
          'tail_handed': '(self)'},
 'Sites': {'KINDS': None,
           '__init__': '(self, ctx: "\'Context\'", handle)',
           'close': '(self)',
           'contexts': "(self) -> 'np.ndarray'",
           'deferred': '(self)',
           'fetch': '(self)',
           'flagged': "(self) -> 'np.ndarray'",
           'info': '(self)',
           'insert': '(self, line, chromosome, start, end, strand, posteriormax, status, meth_lvl, context=None)',
           'mask': "(self) -> 'int'",
           'sort': '(self) -> "\'Sites\'"',
           'sort_info': '(self)',
           'sort_order': "(self) -> 'np.ndarray'",
           'split': '(self) -> "\'dict[str, Sites]\'"',
           'split_ms': '(self)'},
 'SitesParams': {'contexts': None, 'skip_lines': None, 'slab_bytes': None},
 'Tiles': {'ALIGN': None,
           'block_bootstrap': "(self, seed: 'int', n_replicates: 'int')",
           'block_groups': '(self)',
           'block_ms': "(self) -> 'np.ndarray'",
           'close': '(self)',
           'from_parsed': "(cls, ctx: 'Context', sites_list, *, posterior_max_filter, align=False)",
           'info': '(self)',
           'intervals': '(self)',
           'kernel_ms': "(self) -> 'np.ndarray'",
           'layout': '(self)',
           'pairwise': '(self)',
           'pool_columns': '(self)',
           'pool_kernel_ms': "(self) -> 'np.ndarray'",
           'pool_segments': '(self)',
           'runs': '(self)',
           'set_fixed': '(self, size, step=0)',
           'set_intervals': '(self, chromosome, start, end)',
           'set_pools': '(self, chromosome, start, end, pool, n_pools)',
           'stats': '(self)',
           'transitions': '(self)'},
 'Windows': {'__init__': "(self, ctx: 'Context', site_offset, pos, gene_start, gene_end, flags, code, level, *, "
                         'cutoff, step, size, absolute, counts)',
             'close': '(self)',
             'common': '(self)',
             'from_parsed': "(cls, ctx: 'Context', genes: 'Genes', sites_list, *, posterior_max_filter, cutoff, "
                            'cutoff_gene_length=False, step, size, absolute, counts, align=False)',
             'from_sites': "(cls, ctx: 'Context', genes: 'Genes', site_offset, chromosome, start, end, strand, code, "
                           'level, *, cutoff, cutoff_gene_length=False, step, size, absolute, counts)',
             'layout': '(self)',
             'merge_ms': "(self) -> 'np.ndarray'",
             'packed': "(self) -> 'np.ndarray'",
             'packed_device_ptr': "(self) -> 'int'",
             'pairwise': '(self)',
             'stats': '(self)',
             'union': '(self)'},
 'WindowsParams': {'absolute': None,
                   'cutoff': None,
                   'n_downstream': None,
                   'n_gene': None,
                   'n_upstream': None,
                   'size': None,
                   'step': None}}


def test_public_surface_is_unchanged():
    import alphabeta_rs_amd

    names, classes = surface(alphabeta_rs_amd)
    assert names == NAMES
    assert sorted(classes) == sorted(CLASSES)
    for name in CLASSES:
        assert classes[name] == CLASSES[name], name
