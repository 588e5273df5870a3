"""DESIGN.md = tools/design/DESIGN.tpl.md with every @NAME@ replaced by a number read from profiles/r06/ (run from the repo root after the
evidence files have been refreshed: `python tools/design/fill_design.py`).  The prose lives in the template; edit it there."""
import json, re, sys
d='profiles/r06/'
b=json.load(open(d+'bench.json')); m2=b['m2_global256']; n=m2['native_c_abi_world1']; r=b['roofline']; rf=m2['roofline']
o=json.load(open(d+'bench_odometry_frame.json'))['config']['frames_10000_pts']
ll=o['live_loop']; one=ll['one_submission_create_frame']; sep=ll['separate_calls']
u=json.load(open(d+'bench_odometry_under_load.json'))['config']['wirings']['own_context_high_priority']['resident_session']
sm=json.load(open(d+'bench_submap20.json'))['config']
rg=json.load(open(d+'bench_rgbd300k.json')); fe=json.load(open(d+'bench_frontend128k.json'))
ur=json.load(open(d+'bench_under_rocprof.json'))
tr=json.load(open(d+'traffic.json'))
vm=open(d+'voxelmap_time.txt').read()
vmv=[float(x) for x in re.findall(r'insert p50 ([0-9.]+) us',vm)]
ps=m2['predicted_scaling']; src=ps['pair_order_source_major']['cost_model_points']; tgt=ps['pair_order_target_major']['cost_model_points']
cb=b['cpu_baseline']; curve=cb['thread_curve_calls_per_s']
bd=json.load(open(d+'bench_global256_native.json'))['native']['host_breakdown_us']['device_0_caller_thread']
st=one['stage_p50_us']
sw=n['pieces_sweep']
f=lambda x,nd=2: f"{x:.{nd}f}"
sp=lambda x: f"{int(round(x)):,}".replace(',',' ')
nat_alone=json.load(open(d+'bench_global256_native.json'))['native']
cop=n.get('with_device_to_host_copies_behind_the_pieces',{}); onerank=n.get('with_the_one_rank_library_call_every_evaluation',{})
take2=ll['one_submission_as_round5_take2']; nofused=ll['one_submission_without_fused_frame_kernels']; nogate=ll['one_submission_without_gated_pull']; norec=ll['one_submission_without_plan_recycling']
fc=one['inside_frame_create_p50_us_since_entry']
vals={
 'NATIVE_COPIES': f(cop['ms_per_evaluation'],2), 'NATIVE_COPIES_DELTA': f"{cop['ms_per_evaluation']-n['ms_per_evaluation']:.2f}", 'NATIVE_COPIES_AFTER': f(cop['collective_and_copy_out_after_the_kernels_ms'][0]*1e3,0),
 'NATIVE_AFTER': f(n['per_device'][0]['collective_and_copy_out_after_the_kernels_ms']*1e3,0), 'NATIVE_KERNELS': f(n['per_device'][0]['kernels_ms'],2),
 'NATIVE_MINUS_M2': f"{n['ms_per_evaluation']-m2['ms_per_step']:+.2f}", 'ONE_RANK_HOST': f(onerank['library_calls_host_us'],1),
 'FRAME_NOFUSED_NOGATE': f(ll['one_submission_without_fused_frame_kernels_and_gated_pull']['frame_us']['p50'],0),
 'FRAME_TAKE2': f(take2['frame_us']['p50'],0), 'FRAME_NOFUSED': f(nofused['frame_us']['p50'],0), 'FRAME_NOGATE': f(nogate['frame_us']['p50'],0), 'FRAME_NORECYCLE': f(norec['frame_us']['p50'],0),
 'LIN_FIRST': f(st['first_linearisation_new_factor_list'],0), 'LIN_FIRST_NORECYCLE': f(norec['stage_p50_us']['first_linearisation_new_factor_list'],0),
 'PLANS_BUILT': str(one['factor_plans_built']), 'PLANS_RECYCLED': str(one['of_them_in_the_buffers_of_an_evicted_plan']),
 'FC_LAUNCHED': f(fc['pull_kernel_launched'],1), 'FC_PACKED': f(fc['host_conversion_done'],1), 'FC_SEEN': f(fc['completion_word_seen'],1), 'FC_TAIL': f(fc['completion_word_seen']-fc['host_conversion_done'],0),
 'FC_TAIL_BEFORE': '29',
 'FC_PACK_US': f(fc['host_conversion_done']-fc['pull_kernel_launched'],0),
 'ACHIEVED': f(r['achieved']/1000,2), 'ALGO_RATIO': f(r['algorithmic_48B_ratio_to_peak'],2), 'BATCHED': f(b['batched_calls_per_s']/1e6,2),
 'BOUND2': f(src['2']['compute_only_speedup_bound'],2), 'BOUND4': f(src['4']['compute_only_speedup_bound'],2), 'BOUND8': f(src['8']['compute_only_speedup_bound'],2),
 'BOUNDT8': f(tgt['8']['compute_only_speedup_bound'],2), 'BSPEEDUP': sp(b['batched_speedup_vs_cpu_baseline']), 'CPU': sp(cb['value']),
 'CPUMS': f(1e3/cb['value'],2), 'CURVE': ' / '.join(sp(curve[k]) for k in sorted(curve,key=int)), 'FP32FRAC': f(rf['fp32']['frac_of_fp32_vector_peak'],2),
 'FP32TF': f(rf['fp32']['achieved_tflops'],1), 'FRAC629': f(r['frac_of_6.29TBs_copy_rate'],2), 'FRAC': f(r['frac'],2), 'FRAC_M2': f(rf['frac'],2),
 'FRAME_ONE99': f(one['frame_us']['p99'],0), 'FRAME_ONE': f(one['frame_us']['p50'],0), 'FRAME_SEP99': f(sep['frame_us']['p99'],0), 'FRAME_SEP': f(sep['frame_us']['p50'],0),
 'FRAME_STAGES': f"clone + two maps {st['clone_and_two_voxelmaps']:.0f} µs, first linearisation of the new list {st['first_linearisation_new_factor_list']:.0f}, each further one {st['each_further_linearisation']:.0f}, overlap {st['overlap_15_targets']:.0f}, retiring a frame {st['retire_oldest_window_frame']:.0f}",
 'FRONTEND': sp(fe['value']), 'FRONTEND_CPU': f(fe['cpu_baseline']['value'],1), 'K4ROC': f"average of {next(x['calls'] for x in json.load(open(d+'summary.json'))['kernel_trace_by_grid'] if 'vgicp_kernel' in x['kernel'])} launches {tr['kernel_avg_us_rocprof']:.1f} µs, its own bench line {ur['roofline']['kernel_ms']*1e3:.1f} µs, `profiles/r06/summary.json`",
 'K4US': f(r['kernel_ms']*1e3,1), 'M2': f(m2['ms_per_step'],2), 'M2K': f(rf['kernel_ms'],2), 'NATIVE': f(n['ms_per_evaluation'],2),
 'NATIVE_BD': f"pose staging {bd['pose_stage']:.0f} µs + enqueue {bd['enqueue']:.0f} + collective enqueue {bd['collective']:.0f} (all beside running kernels except the first piece's share), {bd['wait']/1e3:.2f} ms waiting for the device, {bd['scan']:.1f} µs for the cost: {bd['total']/1e3:.2f} ms in the call",
 'NATIVE_ALONE': f(json.load(open(d+'bench_global256_native.json'))['native']['ms_per_evaluation'],2), 'NATIVE_ALONE_DELTA': f"{json.load(open(d+'bench_global256_native.json'))['native']['ms_per_evaluation']-m2['synchronous_per_evaluation']['ms_per_evaluation']:+.2f}",
 'NATIVE_DELTA': f"{m2['synchronous_per_evaluation']['native_minus_this_ms']:+.2f}", 'OVBATCH': f(o['keyframe_elimination_loop_one_batch_us'],0),
 'PIECES': ' / '.join(f(sw[k]['ms_per_evaluation'],2) for k in ('1','2') if k in sw)+' / '+f(sw['default']['ms_per_evaluation'],2)+' / '+f(sw['8']['ms_per_evaluation'],2),
 'RGBD': sp(rg['value']), 'SHARDSUM': f(src['8']['shards_sum_ms'],2), 'SPEEDUP': f(b['speedup_vs_cpu_baseline'],1),
 'SUBMAP': f"linearise {sm['bundle_linearize_ms']:.3f} ms per step, LM iteration {sm['lm_iteration_ms']:.2f} ms (round 4: 0.24–0.25 / 0.48)",
 'SYNC': f(m2['synchronous_per_evaluation']['ms_per_evaluation'],2), 'TRAFFIC_MB': f(r['traffic']/1e6,1),
 'UNDERLOAD': f"**{u['p99_ratio']:.1f}×** ({u['idle']['p99_us']:.0f} → {u['under_load']['p99_us']:.0f} µs)", 'VALUE': sp(b['value']),
 'VM10': f"{min(vmv[0],vmv[1]):.0f}–{max(vmv[0],vmv[1]):.0f}", 'VM131': f"{min(vmv[2],vmv[3]):.0f}–{max(vmv[2],vmv[3]):.0f}",
}
# ---- round 6 additions ----
sl=b['single_factor_loop']; tl=sl['resident_timeline_us']; byv=sl['us_per_call_by_variant']; rc=sl['resident_session_cost']
natf=json.load(open(d+'bench_global256_native.json')); virt=natf['virtual_world8']; vb=virt['exchange_behind_the_call']; vs=virt['call_waits_for_the_exchange']
vb0=vb['host_breakdown_us']['device_0_caller_thread']; vbw=vb['host_breakdown_us']['worker_threads_max']
smr=json.load(open(d+'bench_submap20.json'))['roofline']
kr=rg['roofline']; kf=fe['roofline']
m1c=json.load(open(d+'m1_counters.json')); dv=m1c.get('derived',{}); ca=m1c['counters_avg_per_dispatch']
ul=json.load(open(d+'bench_odometry_under_load.json'))['config']['wirings']
hdr=open('include/glim_amd.h').read(); dhdr=open('include/glim_amd_diag.h').read()
n_stable=len(set(re.findall(r"\b(glim_amd_[a-z0-9_]+)\s*\(",hdr))); n_diag=len(set(re.findall(r"\b(glim_amd_[a-z0-9_]+)\s*\(",dhdr)))
def pct_or(x,nd=2): return 'n/a' if x is None else f(x,nd)
def ul_cell(w,mode):
    e=ul[w][mode]; return f"{e['idle']['p99_us']:.1f} → {e['under_load']['p99_us']:.0f} µs ({e['p99_ratio']:.1f}×)"
ul_rows=[('own context, high priority (shipped: the odometry module\'s)','own_context_high_priority','resident session: '),('own context, default priority','own_context','(no session) '),('one shared context (round 3)','shared_context','(no session) ')]
ul_table='| wiring | default switches | `resident=0` |\n|---|---|---|\n'+'\n'.join(f"| {name} | {pre}{ul_cell(w,'resident_session')} | {ul_cell(w,'launch_per_call')} |" for name,w,pre in ul_rows)
mt=ul['own_context_high_priority']['resident_session'].get('mapping_thread',{}); mtl=ul['own_context_high_priority']['launch_per_call'].get('mapping_thread',{})
bursts=one.get('frames_above_1p4x_median',{}); slowest=one.get('slowest_frames',[])
burst_txt=(f"{bursts.get('count',0)} of {bursts.get('of',0)} frames above 1.4 × the median, in {len(bursts.get('runs',[]))} run(s) "+', '.join(f"[frames {r[0]}–{r[1]} at {r[2]:.0f} ms]" for r in bursts.get('runs',[])[:6])+"; the slowest frames' excess sits in "+', '.join(sorted(set(x['excess_in'] for x in slowest)))) if bursts else 'n/a'
p99s=one.get('stage_p99_us',{})
transit=tl['host_round_trip']-tl['device_span']
def counters_txt(c):
    a=c['counters_avg_per_dispatch']; dvv=c.get('derived',{}); cyc=a['SQ_BUSY_CYCLES']/32.0; per_simd=a['SQ_INSTS_VALU']/1024.0
    return (f"{a['SQ_INSTS_VALU']/max(1,a['SQ_WAVES']):.0f} vector instructions per wavefront, {cyc/1e3:.0f} k cycles per launch at {cyc/c['kernel_avg_us_rocprof']/1e3:.2f} GHz, "
            f"one vector instruction issued per {cyc/per_simd:.2f} cycles of a SIMD, wavefronts waiting on a counter {100*(dvv.get('share_of_wave_cycles_waiting_on_any_counter') or 0):.0f} % of their resident "
            f"cycles, L2 hit rate {100*(dvv.get('l2_hit_rate') or 0):.0f} % of {a.get('TCC_REQ_sum',0)/1e6:.0f} M requests"), cyc/per_simd
m2c=json.load(open(d+'m2_counters.json')); m2c_txt,m2_cpv=counters_txt(m2c); m1c_txt,m1_cpv=counters_txt(m1c)
loc=json.load(open(d+'probe/m2_locality_probe.json'))
loc_rep=sum(v['ns_per_1000_visits'] for k,v in loc.items() if k.startswith('sample64_x'))/max(1,sum(1 for k in loc if k.startswith('sample64_x')))
loc_shuf=sum(v['ns_per_1000_visits'] for k,v in loc.items() if k.startswith('sample64_shuffled'))/max(1,sum(1 for k in loc if k.startswith('sample64_shuffled')))
vals.update({
 'CPU_THREADS': str(cb['cores']), 'M2_PTS': sp(m2['config']['mean_points_per_submap']),
 'SYNC_RES': f(byv['resident_session'],1), 'SYNC_SINGLE': f(byv['default_context_no_session'],1), 'SYNC_TWO': f(byv['two_dispatches'],1),
 'SYNC_VERDICT': ('met on this box' if byv['resident_session']<=10.5 else f"not met on this box ({byv['resident_session']:.1f} µs; 10.76–10.84 on the box of the step-major A/B, whose round-5 form would have taken ≈ 13.7)"),
 'TL_PUB': f(tl['leader_published'],2), 'TL_POSE': f(tl['worker_pose_seen_median'],2), 'TL_ROWS': f(tl['worker_row_computed_max'],2), 'TL_PUBROW': f(tl['worker_row_published_max'],2),
 'TL_LOOP': f(tl.get('worker_loop_left_median',0),2), 'TL_LOOPMAX': f(tl.get('worker_loop_left_max',0),2), 'TL_GSUM': f(tl.get('finaliser_group_sums_added',0),2), 'TL_ROT': f(tl.get('finaliser_blocks_rotated',0),2),
 'TL_CLOCK': f(tl.get('shader_clock_mhz',0),0), 'SPEEDUP': f(b['speedup_vs_cpu_baseline'],1),
 'TL_SUM': f(tl['finaliser_rows_summed'],2), 'TL_REC': f(tl['finaliser_record_stored'],2), 'TL_HOST': f(tl['host_round_trip'],2), 'TL_TRANSIT': f(transit,1),
 'COST128': f(rc['batched_128_factor_kernel_ms']['slowdown'],2), 'COST8': f(rc['8_factor_kernel_ms']['slowdown'],2),
 'VIRT_MS': f(vb['ms_per_evaluation'],2), 'VIRT_WAIT_BEHIND': f(vb['host_wait_for_the_exchange_after_the_call_us'],0), 'VIRT_WAIT_SYNC': f(vs['host_wait_for_the_exchange_after_the_call_us'],0),
 'VIRT_EXCH': f"{min(x['exchange_after_the_last_kernel_ms'] for x in vb['per_device']):.1f}–{max(x['exchange_after_the_last_kernel_ms'] for x in vb['per_device']):.1f}",
 'VIRT_HOST': f"post {vb0['post']:.0f} µs, the workers start {vbw['wake']:.0f} µs after the call, pose staging ≤ {max(vb0['pose_stage'],vbw['pose_stage']):.0f}, enqueue ≤ {max(vb0['enqueue'],vbw['enqueue']):.0f}, barrier ≤ {max(vb0['barrier'],vbw['barrier']):.0f}, exchange enqueue ≤ {max(vb0['collective'],vbw['collective']):.0f} µs",
 'SUBMAP_FRAC': f(smr['frac'],2), 'SUBMAP_ALGO': f(smr['algorithmic_48B_ratio_to_peak'],2),
 'KNN_RGBD_US': f(kr['kernel_ms']*1e3,1), 'KNN_RGBD_ROC': pct_or(kr.get('kernel_avg_us_rocprof'),1), 'KNN_RGBD_TRAFFIC': pct_or(kr['traffic']/1e6 if kr.get('traffic') else None,1), 'KNN_RGBD_ALGO': f(kr['algorithmic_bytes_per_launch']/1e6,1), 'KNN_RGBD_FRAC': f(kr['frac'],3),
 'KNN_FE_N': sp(kf['points']), 'KNN_FE_US': f(kf['kernel_ms']*1e3,1), 'KNN_FE_TRAFFIC': pct_or(kf['traffic']/1e6 if kf.get('traffic') else None,2), 'KNN_FE_FRAC': f(kf['frac'],4),
 'FRONT_RETIRE': f(fe['config']['stage_ms']['retire_the_frame_before_last'],3), 'FRONT_LIN': f(fe['config']['stage_ms']['linearize'],3),
 'M1_COUNTERS': m1c_txt,
 'M2_COUNTERS': m2c_txt, 'M1_CPV': f(m1_cpv,2), 'M2_CPV': f(m2_cpv,2), 'M1_ISSUE_PCT': f(100*2.85/m1_cpv,0), 'M2_ISSUE_PCT': f(100*2.74/m2_cpv,0),
 'LOC_ALL': f(loc['all_pairs']['ns_per_1000_visits'],2), 'LOC_REP': f(loc_rep,2), 'LOC_SHUF': f(loc_shuf,2), 'LOC_ONE': f(loc['one_pair_x32640']['ns_per_1000_visits'],2),
 'LOC_GAIN': f(100*(1-loc_rep/loc['all_pairs']['ns_per_1000_visits']),1),
 'FRAME_BURSTS': burst_txt, 'FRAME_P99_STAGES': ', '.join(f"{k.replace('_',' ')} {v:.0f}" for k,v in p99s.items()) if p99s else 'n/a',
 'UL_TABLE': ul_table,
 'UL_MAPPING': (f"{mt.get('loops_per_s_alone',0):.0f} loops/s alone, {mt.get('loops_per_s_beside_the_odometry',0):.0f} beside the odometry's resident session ({mt.get('slowdown',0):.2f}×), {mtl.get('loops_per_s_beside_the_odometry',0):.0f} beside its launch-per-call form ({mtl.get('slowdown',0):.2f}×)") if mt else 'n/a',
 'ABI_STABLE': str(n_stable), 'ABI_DIAG': f"{n_diag} entry points",
})
# ---- the continuous-time GICP factor (tools/ct_gicp_time.py) ----
ct=json.load(open('profiles/ct_gicp/ct_gicp_time.json'))['sources']
for tag,key in (('CT10','pre10k'),('CT131','raw131k')):
    c=ct[key]
    vals.update({tag+'_N':sp(c['source_points']), tag+'_LIN':f(c['ct_linearize']['p50_us'],1), tag+'_ERR':f(c['ct_error']['p50_us'],1),
                 tag+'_GICP':f(c['gicp_linearize']['p50_us'],1), tag+'_RATIO':f(c['ct_over_gicp_linearize'],2), tag+'_FRAME':f(c['lm_frame_8_iterations']['p50_us']/1e3,2),
                 tag+'_BUCKETS':str(c['buckets'])})
# ---- the device iVox (tools/ivox_time.py) ----
iv=json.load(open('profiles/ivox/ivox_time.json')); ivf=iv['ct_factor']
vals.update({'IVX_MAP_POINTS':sp(iv['map']['num_points']), 'IVX_MAP_VOXELS':sp(iv['map']['num_voxels']), 'IVX_SRC':sp(iv['source_points']),
             'IVX_INS':f(iv['insert_sweep']['p50_us'],0), 'IVX_INS_RAW':f(iv['insert_raw_131072']['p50_us'],0),
             'IVX_IDX':f(iv['index_rebuild_accumulated_cloud']['p50_us'],0), 'IVX_INS_RATIO':f(iv['insert_over_index_rebuild'],2),
             'IVX_LIN1':f(ivf['ivox_mode1']['linearize']['p50_us'],0), 'IVX_LIN7':f(ivf['ivox_mode7']['linearize']['p50_us'],0),
             'IVX_LIN27':f(ivf['ivox_mode27']['linearize']['p50_us'],0), 'IVX_LIN_IDX':f(ivf['index']['linearize']['p50_us'],0),
             'IVX_LIN_RATIO':f(iv['mode1_linearize_over_index_linearize'],2), 'IVX_ERR1':f(ivf['ivox_mode1']['error']['p50_us'],0),
             'IVX_FRAME':f(iv['frame_8_iterations_deskew_covariances_insert']['p50_us']/1e3,2)})
# ---- the CT-GICP frame alignment (tools/ct_align_time.py) ----
cta=json.load(open('profiles/ct_align/ct_align_time.json'))
vals.update({'CTA_SRC':sp(cta['source_points']), 'CTA_TGT':sp(cta['target_points'])})
for tag,key in (('CTA_IX','index'),('CTA_IV','ivox_mode1')):
    c=cta['targets'][key]
    vals.update({tag+'_DEV':f(c['device']['p50_us']/1e3,2), tag+'_HOST':f(c['host_loop']['p50_us']/1e3,2), tag+'_ROUNDS':str(c['rounds']),
                 tag+'_ROUND':f(c['device_per_round_us'],0), tag+'_RATIO':f(c['host_over_device'],2)})
# ---- the VGICP fine registration (tools/vgicp_align_time.py) ----
import os
vga_path='profiles/vgicp_align/vgicp_align_time.json'
if os.path.exists(vga_path):
    vga=json.load(open(vga_path))['shapes']
    cell=lambda r,k: f"{r[k]['wall_ms_p50']:.2f} ms for {r[k]['rounds']} rounds, {r[k]['factor_evaluations_used']} evaluations used ({r[k]['wall_us_per_round']:.0f} µs per round, {r[k]['wall_us_per_evaluation_used']:.0f} µs per evaluation used)"
    vals['VGA_MEASURED']=(f"one box, not repeated, the variants alternating in one process (`tools/vgicp_align_time.py`, `profiles/vgicp_align/vgicp_align_time.json`; a {sp(vga[0]['source_points'])}-point source against the map of a {sp(vga[0]['target_points'])}-point scan, the default parameters).  "
        +'  '.join(f"B = {r['B']}: device batch {cell(r,'device_batch')}; host-driven loop over `linearize_poses` {cell(r,'host_loop')}." for r in vga)
        +"  The two loops do not run the same number of evaluations (the device enqueues every round up front, the host loop stops with the last problem): the per-round figures are the comparable ones.  No speedup is claimed.")
else:
    vals['VGA_MEASURED']="nothing yet.  `tools/vgicp_align_time.py` writes `profiles/vgicp_align/vgicp_align_time.json` (the device batch against the host-driven loop over `NonlinearFactorSetGPU.linearize_poses`, B = 1 / 16, a 12 000-point source against a 131 072-point map, totals and per-evaluation figures, the variants alternating in one process); until that file exists every statement about the speed of this path is UNMEASURED."
# ---- the sub-map bundle optimisation (tools/bundle_align_time.py) ----
bun_path='profiles/bundle_align/bundle_align_time.json'
if os.path.exists(bun_path):
    bun=json.load(open(bun_path))
    d,h,r=bun['device_loop'],bun['host_iteration'],bun['round_split']
    vals['BUNDLE_MEASURED']=(f"one box, not repeated, the variants alternating in one process (`tools/bundle_align_time.py`, `{bun_path}`; the configs[2] bundle: {bun['keyframes']} keyframes of {sp(bun['points_per_cloud'])} points, {bun['factors']} factors, a prior on keyframe 0, the default parameters).  "
        f"Device loop {d['wall_ms_p50']:.2f} ms for {bun['rounds_enqueued']} enqueued rounds of which {d['rounds_that_ran']} ran ({d['status']}, {d['iterations']} iterations): {d['wall_us_per_round_that_ran']:.0f} µs per round that ran.  "
        f"The host-driven iteration over the same set (synchronous `linearize` + `error`, bench.py's `lm_iteration_ms`) {h['lm_iteration_ms_p50']:.2f} ms, {h['for_the_same_rounds_ms']:.2f} ms for as many rounds, the host's assembly and solve not counted.  "
        f"With exactly the rounds it needs enqueued the call takes {bun['device_loop_exact_budget']['wall_ms_p50']:.2f} ms, with round 0 alone {bun['device_loop_round_0_only']['wall_ms_p50']:.2f} ms (the fixed part: arguments, the transient plan, uploads), so a trial round costs {r['trial_round_us']:.0f} µs: "
        f"the 380 factors' evaluation alone {r['factor_round_us_p50']:.0f} µs; the rest (the decide kernel and the launch gaps), by difference, {r['rest_of_a_round_us_by_difference']:.0f} µs.  "
        "As measured the device round is SLOWER than the host-driven iteration: the one-workgroup decide kernel is about three quarters of a round.  Where its time goes (the serial item lists of the assembly read from device memory, the 120 barriers of the factorisation, the `noinline` SE(3) items) has not been profiled; unrolling the factorisation's dot loops by eight changed nothing measurable.  What the call saves today is the host's assembly and solve and the per-trial round trips, not time on this bundle; no speedup is claimed.")
else:
    vals['BUNDLE_MEASURED']="nothing yet.  `tools/bundle_align_time.py` writes `profiles/bundle_align/bundle_align_time.json` (the device loop on the configs[2] bundle against the host-driven iteration over `linearize` and `error` of the same set, and the split of a round between the factor kernels and the decide kernel, the variants alternating in one process); until that file exists every statement about the speed of this path, the one-workgroup FP64 Cholesky included, is UNMEASURED."
# ---- the scan-to-keyframes VGICP registration (tools/keyframe_align_time.py) ----
kfa_path='profiles/keyframe_align/keyframe_align_time.json'
if os.path.exists(kfa_path):
    kfa=json.load(open(kfa_path))['shapes']
    ran=lambda r,k: r[k].get('rounds_that_ran_a_problem', r[k]['rounds'])
    cell=lambda r,k: f"{r[k]['wall_ms_p50']:.2f} ms for {r[k]['rounds']} rounds of which {ran(r,k)} ran, {r[k]['factor_evaluations_used']} factor evaluations used ({r[k]['wall_ms_p50']*1e3/ran(r,k):.0f} µs per round that ran)"
    vals['KEYFRAME_MEASURED']=(f"one box, not repeated, the variants alternating in one process (`tools/keyframe_align_time.py`, `{kfa_path}`; a {sp(kfa[0]['source_points'])}-point source against {kfa[0]['targets_per_problem']} maps of {sp(kfa[0]['target_points'])}-point scans, the default parameters).  "
        +'  '.join(f"B = {r['B']} ({r['factors']} factors): device batch {cell(r,'device_batch')}; host-driven loop over `linearize_poses` {cell(r,'host_loop')}." for r in kfa)
        +"  The device enqueues every round up front and the host loop stops with the last problem, so both times are divided by the rounds that ran a problem; the enqueued rounds that found every problem finished are in the device's time.  No speedup is claimed.")
else:
    vals['KEYFRAME_MEASURED']="nothing yet.  `tools/keyframe_align_time.py` writes `profiles/keyframe_align/keyframe_align_time.json` (the device batch against the host-driven loop over `NonlinearFactorSetGPU.linearize_poses` of the same 34 B pairs, B = 1 / 8, a 12 000-point source against 17 × 2 maps of 131 072-point scans, totals and per-round figures, the variants alternating in one process); until that file exists every statement about the speed of this path is UNMEASURED."
# ---- the plane bundle-adjustment tool (tools/plane_ba_time.py) ----
pba_path='profiles/plane_ba/plane_ba_time.json'
if os.path.exists(pba_path):
    pba=json.load(open(pba_path)); pd,ph=pba['device'],pba['numpy_restatement']
    vals['PLANE_BA_MEASURED']=(f"one box, one run (`tools/plane_ba_time.py`, `{pba_path}`; {pba['submaps']} sub-maps of {sp(pba['points_per_submap'])} points, a wall through the centre, r₀ = {pba['r0']:g} selecting {sp(pba['selected_at_r0'])} points in {pba['frames_in_factor']} frames; "
        f"synchronous calls timed on the host, median of {pba['repeats']}).  Device: select {pd['select_ms']:.2f} ms, statistics {pd['stats_ms']:.2f} ms, the whole radius search ({pba['auto_radius']['evaluations']} evaluations, one synchronisation) {pd['auto_radius_ms']:.2f} ms, "
        f"factor creation from the ball {pd['factor_create_from_ball_ms']:.2f} ms, one linearize {pd['linearize_ms']:.3f} ms, one error {pd['error_ms']:.3f} ms.  "
        f"The NumPy restatement of the same steps: select {ph['select_ms']:.0f} ms, select + statistics {ph['select_and_stats_ms']:.0f} ms, the radius search {ph['auto_radius_ms']:.0f} ms, the factor in point form {ph['factor_linearize_point_form_ms']:.0f} ms.  "
        "Every device figure includes the upload of the sub-map descriptors and the transform pass over all points; nothing beyond these two programs is compared and no speed-up was promised in advance.")
else:
    vals['PLANE_BA_MEASURED']="nothing yet.  `tools/plane_ba_time.py` writes `profiles/plane_ba/plane_ba_time.json` (24 sub-maps of 65 536 points, r₀ = 1: select, statistics, the whole radius search, factor creation and one linearize beside the NumPy restatement of the same steps); until that file exists every statement about the speed of this path is UNMEASURED."
# ---- the map editor (tools/map_edit_time.py) ----
me_path='profiles/map_edit/map_edit_time.json'
if os.path.exists(me_path):
    me=json.load(open(me_path)); st=me['steps']
    both=lambda k: f"{st[k]['device_ms']:.2f} ms against {st[k]['numpy_restatement_ms']:.0f} ms"
    rs,rb=me['region_growing_small_window'],me['region_growing_default_window']
    vals['MAP_EDIT_MEASURED']=(f"one box, one run (`tools/map_edit_time.py`, `{me_path}`; {me['submaps']} sub-maps of {sp(me['points_per_submap'])} points, a wall through the picked point; "
        f"synchronous calls timed on the host, median of {me['repeats']}, the NumPy restatement of the same step beside each, median of {me['restatement_repeats']}, in one process).  Device against restatement: "
        f"box ({sp(me['selected']['box'])} points selected) {both('box')}, sphere {both('sphere')}, window ({sp(me['selected']['window'])}) {both('window')}, radius {me['radius']:g} ({sp(me['selected']['radius'])}) {both('radius')}, "
        f"outliers in that radius ({sp(me['selected']['outliers'])}) {both('outliers')}, region growing in a 1 m window ({sp(rs['num_candidates'])} candidates, cluster {sp(rs['count'])}, {rs['rounds']} rounds) {both('region_growing_small_window')}.  "
        f"Device only: region growing in the editor's default window ({sp(rb['num_candidates'])} candidates, cluster {sp(rb['count'])}, {rb['rounds']} rounds in chunks of {me['rounds_per_look']}) {st['region_growing_default_window']['device_ms']:.2f} ms "
        f"({st['region_growing_default_window']['device_ms']*1e3/max(rb['rounds'],1):.0f} µs per round, the selection, sort and read-backs included), removing that cluster from the sub-maps it touches {st['remove_selected']['device_ms']:.2f} ms.  "
        "Every compared step returned the restatement's pairs.  The restatement is single-threaded NumPy (its region growing a dense distance matrix): the figures describe these two programs, nothing was profiled, and no speed-up is claimed.")
    if 'min_cut' in me:
        mc=me['min_cut']
        vals['MAP_EDIT_MEASURED']+=(f"  Min-cut at the editor's defaults (foreground {mc['params']['foreground_mask_radius']:g} m, background {mc['params']['background_mask_radius']:g} m, k {mc['params']['k_neighbors']}) on the same workload, a run of its own: "
            f"{sp(mc['num_candidates'])} candidates, {sp(mc['num_edges'])} edges, {sp(mc['num_foreground'])} foreground and {sp(mc['num_background'])} background points, flow {sp(mc['flow'])} units, segment {sp(mc['count'])} points, "
            f"{mc['rounds']} push rounds in {mc['looks']} chunks, status {mc['status']}: the device call {mc['device_ms']:.0f} ms (median of {mc['device_repeats']}; selection, kNN, sorts and every read-back included; {mc['device_ms']/max(mc['looks'],1):.0f} ms per chunk with its relabelling) "
            f"beside {mc['scipy_maximum_flow_ms']/1e3:.1f} s inside `scipy.sparse.csgraph.maximum_flow` on the graph the device built and downloaded (single-threaded; building its matrix and reading the cut off the residuals not counted); "
            f"the two results are {'equal' if mc['equal'] else 'NOT equal'} (flow and set).  A description of two programs: the issue set no time target, and no round of this solver has been profiled.")
else:
    vals['MAP_EDIT_MEASURED']="nothing yet.  `tools/map_edit_time.py` writes `profiles/map_edit/map_edit_time.json` (24 sub-maps of 65 536 points: the four selections, the outliers, region growing and the removal beside the NumPy restatement of the same steps, alternating in one process); until that file exists every statement about the speed of this path is UNMEASURED."
# ---- the graph optimiser over pose, velocity and bias nodes (tools/nav_graph_time.py) ----
nav_path='profiles/nav_graph/nav_graph_time.json'
if os.path.exists(nav_path):
    nav=json.load(open(nav_path))
    cell=lambda r: f"{r['wall_ms_p50']:.2f} ms for the call, {r['rounds_that_ran']} rounds ran ({r['status']}, {r['iterations']} iterations), {r['round_ms']:.2f} ms a round"
    s20,g36=nav['submap20'],nav['global36']['terms_only']
    vals['NAV_MEASURED']=(f"one box, one run (`{nav_path}`, the default parameters).  The sub-mapping-shaped graph over 20 frames ({s20['terms_only']['nodes']} nodes, {s20['terms_only']['rows']} rows, "
        f"{s20['terms_only']['imu_terms']} IMU terms): terms only {cell(s20['terms_only'])}; with the {s20['with_two_hop_factors']['factors']} two-hop VGICP factors {cell(s20['with_two_hop_factors'])}.  "
        f"The global-mapping-shaped graph over 36 sub-maps ({g36['nodes']} nodes, {g36['rows']} rows, {g36['imu_terms']} IMU terms), terms only: {cell(g36)}.  "
        +(f"The trial round of `graph_align` without new terms at N = 64 (`tools/graph_align_time.py`), two processes each, alternating with the parent commit: "
          f"{nav['graph_align_round_time_n64']['this'][0]:.3f} and {nav['graph_align_round_time_n64']['this'][1]:.3f} ms against the parent's {nav['graph_align_round_time_n64']['parent'][0]:.3f} and {nav['graph_align_round_time_n64']['parent'][1]:.3f} ms, "
          f"whose own spread is {100*nav['graph_align_round_time_n64']['margin_the_parents_own_spread']:.1f} %.  " if 'graph_align_round_time_n64' in nav else "")
        +"Nothing was profiled and no speed-up is claimed.")
else:
    vals['NAV_MEASURED']="nothing yet.  `tools/nav_graph_time.py` writes `profiles/nav_graph/nav_graph_time.json` (a 20-frame sub-mapping-shaped graph with and without the two-hop VGICP factors, a 36-sub-map global-mapping-shaped graph); until that file exists every statement about the speed of this path is UNMEASURED."
s=open('tools/design/DESIGN.tpl.md').read()
missing=set(re.findall(r'@([A-Z0-9_]+)@',s))-set(vals)
assert not missing, missing
for k,v in vals.items(): s=s.replace('@'+k+'@',v)
if '--check' in sys.argv:  # tests/test_abi_cpu.py: DESIGN.md is exactly the template filled from the committed evidence
    sys.exit(0 if open('DESIGN.md').read()==s else 1)
open('DESIGN.md','w').write(s)
for k in sorted(vals): print(k,'=',vals[k])
