// gf_tracker.hip — C-ABI front end (include/groundfusion_hip.h): host orchestration of the HIP tracker.
//
// Mirrors FeatureTracker (vins_estimator/src/featureTracker/feature_tracker.{h,cpp}) for `batch`
// independent sequences on one GPU stream; a call advances the sequences it lists (track_core), the lock-step entry points list them all.  The bookkeeping the
// reference keeps in C++ (ids, track_cnt, n_id, maps for velocity, setMask's walk, the camera model) is gf_track_host.hpp, plain C++ per sequence; all image work
// (pyramids, Scharr, LK forward/reverse, mask rasterisation, Shi-Tomasi, candidate sort and min-distance selection, depth sampling) runs in the kernels of
// gf_lk_kernels.hpp / gf_detect_kernels.hpp.  This file owns the handle, its tables and streams, and the order of a frame.  track_core runs these stages:
//   publish        the call's list and frame table where the first kernels read them, over the bus or by copy
//   launch_front   conversion, equalisation, pyramid; the frames_unaligned count; then the depth registration of the sequences that have one (launch_depth_reg)
//   run_lk         stage_points per sequence, tables down, one or two LK launches, tables up; the host waits
//   redo_fallback  LK from scratch for the predicted sequences with fewer than 10 forward successes
//   book_after_lk  per sequence on the pool (after_lk): reduction by status, setMask, the corners wanted
//   run_detect     tables down, detector, selection, the lift of the sequences whose camera is no pinhole (launch_lift), tables up; the host waits
//   read_profile, check_candidates   event times; the candidate capacity and the selection-branch counters
//   book_after_detect  per sequence on the pool (after_detect): addPoints, lift, velocities, roll-over, packing; then the stats
// There is no CPU fallback: without a HIP device every entry point fails with GF_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <sched.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/groundfusion_hip.h"
#include "gf_camera_models.hpp"
#include "gf_comm.hpp"
#include "gf_detect_kernels.hpp"
#include "gf_lk_kernels.hpp"
#include "gf_stereo_kernels.hpp"
#include "gf_stereo_depth.hpp"
#include "gf_copy_list.hpp"
#include "gf_depth_reg_stage.hpp"
#include "gf_reject_f_stage.hpp"
#include "gf_frame_ref.hpp"
#include "gf_host_cpus.hpp"
#include "gf_hip_own.hpp"
#include "gf_pixfmt.hpp"
#include "gf_roi.hpp"
#include "gf_seq_cfg.hpp"
#include "gf_seq_format.hpp"
#include "gf_seq_size.hpp"
#include "gf_track_draw.hpp"
#include "gf_track_host.hpp"

namespace gf {

// gf_clahe.hip: cv::CLAHE::apply on `batch` contiguous frames (gf_tracker_cfg.equalize)
size_t clahe_lut_bytes(int batch, int tiles_x, int tiles_y);
int clahe_launch(const uint8_t* d_src, uint8_t* d_dst, uint8_t* d_lut, int batch, int w, int h, double clip_limit, int tiles_x, int tiles_y, hipStream_t stream);
// gf_cvt.hip: cv_bridge::toCvCopy(msg, MONO8) on `batch` frames, src_pitch bytes from row to row (gf_tracker_cfg.pixel_format)
int cvt_launch(const uint8_t* d_src, size_t src_pitch, int format, uint8_t* d_dst, int batch, int w, int h, hipStream_t stream);
// the table forms of the two (gf_frame_ref.hpp): frame b of the source lies at refs[b]
int clahe_launch_refs(const gf_frame_ref* d_refs, uint8_t* d_dst, uint8_t* d_lut, int batch, int w, int h, double clip_limit, int tiles_x, int tiles_y, hipStream_t stream);
int cvt_launch_refs(const gf_frame_ref* d_refs, const gf_frame_ref* h_refs, int format, uint8_t* d_dst, int batch, int w, int h, hipStream_t stream, int* n_bytes);
// one format per frame (gf_tracker_set_seq_format): entry b at d_refs[b] in d_formats[b], -1 = skip; h_*: the same tables as the host reads them
int cvt_launch_mixed(const gf_frame_ref* d_refs, const int* d_formats, const gf_frame_ref* h_refs, const int* h_formats, uint8_t* d_dst, int batch, int w, int h, hipStream_t stream);
// gf_track_draw.hip: the track image of `count` frames, one per entry of d_jobs (gf_track_draw.hpp), in one launch
int draw_track_launch(const gfdraw::DrawJob* d_jobs, int count, int w, int h, hipStream_t stream);
// gf_camera.hip: liftProjective of the listed entries' cameras (gf_tracker_set_seq_camera), one launch
int camera_lift_launch(const gfcam::LiftArgs& A, int max_n, hipStream_t stream);
// gf_stereo_depth.hip: the depth the matches of the listed positions determine (gf_tracker_set_seq_stereo_depth), one launch
int stereo_depth_launch(const gfsd::Args& A, int max_n, hipStream_t stream);
constexpr double kClaheClip = 40.0;   // cv::createCLAHE() defaults (rosNodeTest.cpp:258)
constexpr int kClaheTiles = 8;

static thread_local std::string g_err;
int set_err(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_err = buf;
    return code;
}

// Small persistent pool for the per-sequence host bookkeeping (sequences are independent).  GF_HOST_THREADS overrides the size.
class HostPool {
  public:
    // device: the pool's threads go onto the cores of that GPU's NUMA node (8 ranks on one host: every rank's bookkeeping next to its own GPU and memory)
    explicit HostPool(int n, int device) {
        for (int i = 0; i < n; i++) workers_.emplace_back([this, device] { gf::pin_thread_to_device_node(device); run(); });
    }
    ~HostPool() {
        { std::lock_guard<std::mutex> l(m_); stop_ = true; gen_++; }
        cv_.notify_all();
        for (auto& t : workers_) t.join();
    }
    // calls fn(b) for b in [0, n); the calling thread takes part
    void parallel_for(int n, const std::function<void(int)>& fn) {
        if (workers_.empty() || n < 8) { for (int b = 0; b < n; b++) fn(b); return; }
        { std::lock_guard<std::mutex> l(m_); fn_ = &fn; n_ = n; next_ = 0; active_ = (int)workers_.size(); gen_++; }
        cv_.notify_all();
        work();
        std::unique_lock<std::mutex> l(m_);
        done_.wait(l, [this] { return active_ == 0; });
        fn_ = nullptr;
    }
  private:
    void work() { for (;;) { const int b = next_.fetch_add(1); if (b >= n_) break; (*fn_)(b); } }
    void run() {
        unsigned long long seen = 0;
        for (;;) {
            { std::unique_lock<std::mutex> l(m_); cv_.wait(l, [&] { return gen_ != seen; }); seen = gen_; if (stop_) return; }
            work();
            { std::lock_guard<std::mutex> l(m_); if (--active_ == 0) done_.notify_one(); }
        }
    }
    std::vector<std::thread> workers_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const std::function<void(int)>* fn_ = nullptr;
    std::atomic<int> next_{0};
    int n_ = 0, active_ = 0;
    unsigned long long gen_ = 0;
    bool stop_ = false;
};

static int build_geom(int w, int h, PyrGeom& G) {
    memset(&G, 0, sizeof G);
    int lw = w, lh = h;
    size_t off = 0;
    int level = 0;
    for (; level < kMaxLevels; level++) {
        LevelGeom& g = G.lv[level];
        g.w = lw; g.h = lh; g.stride = lw + 2 * kPad;
        const size_t rows = lh + 2 * kPad;
        g.img_off = (int)(off + (size_t)kPad * g.stride + kPad);
        off += rows * g.stride;
        off = (off + 255) & ~(size_t)255;
        lw = (lw + 1) / 2; lh = (lh + 1) / 2;
        if (lw <= kWin || lh <= kWin) { level++; break; }  // buildOpticalFlowPyramid stop rule
    }
    G.nlevels = level;
    G.img_bytes = off;
    return GF_OK;
}

}  // namespace gf

using namespace gf;

struct gf_tracker {
    gf_tracker_cfg cfg;
    PyrGeom G;
    DiskTable disk;
    int B = 0, cap = 0, cand_cap = 0, sort_cap = 0;
    bool copy_lists = true;   // GF_TRACKER_COPIES=1: one hipMemcpyAsync per table instead of the copy-list kernels
    bool pyr_head = true;     // GF_PYR_HEAD=0: levels 0 and 1 of the pyramid as two kernels (read when the tracker is created, as the other switches)
    bool select_topk = true;  // GF_SELECT_TOPK=0: every frame's corners through the sort
    int lk_points = 1;        // points per wavefront of the LK kernel: 1 (lk_track_kernel), 2 or 4 (lk_track_mp_kernel, round 6); GF_LK_POINTS
    bool profiling = false;
    // Members are destroyed in reverse order: the pool (last member) is joined before anything its threads could touch goes, the buffers go before the events and streams.
    Stream stream, copy_stream;   // copy_stream, ev_copy: gf_tracker_prefetch_batch (created on first use)
    Event ev[9];   // ev[7]: end of the equalisation (cfg.equalize); ev[8]: end of the colour / raw conversion (cfg.pixel_format)
    int ch = 1;    // bytes per pixel of the frames the handle is given (cfg.pixel_format); d_raw / d_raw2 hold them in that format
    Event ev_copy[2];
    gf_tracker_stats stats{};
    std::vector<SeqState> seq;
    // device
    DevBuf<uint8_t> d_img, d_raw, d_mask, d_status, d_fwd_status, d_seqmask;
    DevBuf<uint8_t> d_eq, d_eq_lut;   // cfg.equalize: the equalised frames the pyramid reads, and the CLAHE tile LUTs
    DevBuf<uint8_t> d_cvt;            // cfg.pixel_format: the MONO8 frames converted from the caller's colour or raw frames, which equalisation and pyramid read
    DevBuf<int> d_npts, d_cand_count, d_want, d_ncenters, d_out_n;
    // the call's sequence list as the kernels read it (cur_of, gf_lk_kernels.hpp): written into the page-locked h_cur, which the pyramid kernels read over the bus
    // (they are launched before anything is copied), and carried to d_cur for LK by the copy list in front of it
    DevBuf<int> d_cur; PinBuf<int> h_cur;
    DevBuf<int> d_det; PinBuf<int> h_det;   // the detector's form of the list (DetectArgs::frame_of): the same entry, or -1 where the sequence wants no corners
    std::vector<int> ident;          // 0 .. batch-1: the list of the lock-step entry points
    std::vector<uint8_t> listed;     // scratch of check_list
    DevBuf<uint16_t> d_depth, d_depth_out, d_out_depth;
    // gf_tracker_prefetch_batch: the next frame's images on their way to the second pair of frame buffers while the current frame's kernels run
    DevBuf<uint8_t> d_raw2; DevBuf<uint16_t> d_depth2;
    int pf_head = 0, pf_count = 0;   // FIFO of staged frames over the two pairs (0: d_raw / d_depth, 1: d_raw2 / d_depth2): oldest pair, number staged (0..2)
    std::vector<int> pf_seq[2];      // the sequences each staged frame holds, in the order of its images (two staged frames may name different sets)
    bool pf_depth[2] = {false, false};
    std::vector<const uint16_t*> pf_hdepth[2]; int pf_hdstride[2] = {0, 0};   // the staged frames' depth images (host; sampled by track_core, never copied)
    DevBuf<float2> d_prev_pts, d_init_pts, d_cur_pts, d_out_pts;
    DevBuf<unsigned> d_counters, d_maxkey;
    DevBuf<float> d_eig;
    DevBuf<unsigned long long> d_cand;
    DevBuf<int2> d_centers;
    // pinned host mirrors
    PinBuf<int> h_npts, h_want, h_ncenters, h_out_n, h_cand_count;
    PinBuf<float2> h_prev_pts, h_init_pts, h_cur_pts, h_out_pts;
    PinBuf<uint8_t> h_status, h_fwd_status, h_seqmask;
    PinBuf<uint16_t> h_depth_out, h_out_depth;
    PinBuf<unsigned> h_counters;
    PinBuf<int2> h_centers;
    size_t eig_stride = 0, mask_stride = 0;
    size_t select_lds = 0;
    // The sequences' regions of interest (gf_roi.hpp; gf_tracker_set_roi*), addressed by SEQUENCE like seq[] and the pyramid pairs.  Everything here is obtained by the
    // first setter of the handle, never by gf_tracker_create: a handle that sets none allocates, copies and launches exactly what it did before there were any.
    // d_roi: [B][roi_words] words the detector ANDs into its allow word, all-ones for a sequence that has no region (the AND changes nothing).  roi_bits: the same
    // words on the host, which setMask's walk reads (set_mask_host); roi_has[seq]: whether the sequence has one (0: the walk skips the test).
    DevBuf<uint32_t> d_roi; DevBuf<int> d_roi_seq;
    std::vector<uint32_t> roi_bits; std::vector<uint8_t> roi_has;
    size_t roi_words = 0;
    // The sequences' exclusion boxes (gf_roi.hpp; gf_tracker_set_boxes_some), obtained by the first box setter of the handle.  From then on d_roi holds the words of
    // R_eff = R_base AND NOT union(boxes), written by roi_boxes_kernel, and d_roi_base the base words the setters of R pack (the table they wrote into d_roi before):
    // next frame's boxes compose with the same base.  roi_bits stays the host's copy of the BASE words; setMask's walk and gf_tracker_get_roi test a pixel against
    // it and boxes[seq] (gfroi::allowed with a list), so no table is rebuilt on or copied to the host for a list of boxes.  h_box_stage / d_box_stage: the jobs of one
    // setter and their boxes, [B] RoiBoxJob then [B x GF_MAX_BOXES_PER_SEQ] gf_box; ev_boxes: behind the kernel that read them last, so that a second setter
    // between two track calls does not write under it (box_pending: one left since the stream was last drained).
    std::vector<std::vector<gf_box>> boxes;
    DevBuf<uint32_t> d_roi_base;
    DevBuf<uint8_t> d_box_stage; PinBuf<uint8_t> h_box_stage;
    Event ev_boxes; bool box_pending = false;
    // The sequences' own parameters (gf_seq_cfg.hpp; gf_tracker_set_seq_cfg), the fourth thing addressed by SEQUENCE.  par[seq] is what is in force, the handle's cfg
    // until a setter says otherwise (host memory only).  The rest is obtained by the first setter of the handle, as the region of interest's tables are: the circle
    // tables of the sequences' min_dist -- seq_disk on the host for setMask's walk, d_seq_disk for the detector -- and the two lists that carry min_dist and
    // flow_back to the selection and LK kernels by list position with the call's other hand-over tables.
    std::vector<gf_tracker_seq_cfg> par;
    std::vector<DiskTable> seq_disk; DevBuf<DiskTable> d_seq_disk;
    DevBuf<int> d_seq_md; PinBuf<int> h_seq_md;
    DevBuf<uint8_t> d_seq_fb; PinBuf<uint8_t> h_seq_fb;
    // Frames by reference (gf_frame_ref.hpp; the _refs entry points): the call's table, [0, B) the gray frames and [B, 2 B) the depth frames by list position.
    // Obtained by the first _refs call of the handle, like the tables above.  It travels like the list: the first kernel of a call reads the page-locked h_refs
    // over the bus, the copy list in front of LK / the detection carries it to d_refs for the depth samples of those kernels.
    DevBuf<gf_frame_ref> d_refs; PinBuf<gf_frame_ref> h_refs;
    // The track image (gf_track_draw.hpp; gf_tracker_set_show_track), obtained by the first call that turns a sequence's switch on.  d_draw_prims: [B][4 cap]
    // primitives by SEQUENCE, a sequence's row written when its picture is first asked for after a frame (SeqState::draw_sent) through its row of the page-locked
    // h_draw_prims.  The jobs of a call by list position.  d_draw_host: the staging image of gf_tracker_track_image, obtained by its first call.
    DevBuf<gfdraw::Prim> d_draw_prims; PinBuf<gfdraw::Prim> h_draw_prims;
    DevBuf<gfdraw::DrawJob> d_draw_jobs; PinBuf<gfdraw::DrawJob> h_draw_jobs;
    DevBuf<uint8_t> d_draw_host;
    // A pixel format and an equalise switch per sequence (gf_seq_format.hpp; gf_tracker_set_seq_format), the fifth thing addressed by SEQUENCE.  fmt[seq] is what
    // is in force, the handle's cfg until a setter says otherwise (host memory only); fmt_any: a setter has given a sequence values of its own.  Everything else is
    // obtained by the setters, as the tables above are: d_cvt / d_eq / d_eq_lut where gf_tracker_create did not need them, d_raw (and d_raw2) grown to raw_ch bytes
    // per pixel, the widest format in force, and the table of a mixed call: [B] conversion sources, [B] equalisation sources (dense), [B] pyramid sources, then
    // [B] formats as the conversion kernel reads them.  It travels like the list and the frame table: page-locked, read over the bus by the three stages.
    std::vector<gf_tracker_seq_format> fmt;
    bool fmt_any = false;
    int raw_ch = 1;
    gfseqfmt::Plan plan;                     // of the call in progress (plan_call)
    std::vector<gf_frame_ref> plan_frames;   // scratch: where the caller's frames of that call lie
    DevBuf<uint8_t> d_mix; PinBuf<uint8_t> h_mix;
    // A camera model per sequence (gf_camera_models.hpp; gf_tracker_set_seq_camera), the sixth thing addressed by SEQUENCE.  Everything here is obtained by the
    // first setter that gives a sequence a model other than PINHOLE; a pinhole stays the eight fields of par[seq] and is lifted on the host as ever.  cam_on[seq]:
    // the sequence has such a model, cam_model / cam[seq] as it was set / as the formulas read it, d_cams the same table on the device (a row written by the
    // setter).  Per call, by list position: cam_of (the sequence, or -1 for a pinhole one, which the kernel skips) and the two tables of lifted pairs, for the rows
    // of LK's points and of the new corners, which come up with the call's last copies.  A sequence that is lifted on the host (lifts_on_device false) uses none
    // of the per-call tables: after_detect lifts it with the same header.
    int lift_mode = -1;   // GF_CAMERA_LIFT_HOST: unset -1 (each model's measured default: SCARAMUZZA on the host, every other model on the device), 0 all on the device, 1 all on the host
    long long lift_launches = 0, lift_sequences = 0;   // gf_tracker_get_camera_lift_stats
    bool lifts_on_device(int q) const {   // sequence q is lifted by the call's launch of camera_lift_kernel
        if (!d_cams.p || !cam_on[q]) return false;
        return lift_mode < 0 ? cam_model[q].model != GF_CAMERA_SCARAMUZZA : lift_mode == 0;
    }
    std::vector<uint8_t> cam_on; std::vector<gf_camera_model_ex> cam_model; std::vector<gfcam::Camera> cam;
    DevBuf<gfcam::Camera> d_cams;
    DevBuf<int> d_cam_of; PinBuf<int> h_cam_of;
    DevBuf<float2> d_un_lk, d_un_out; PinBuf<float2> h_un_lk, h_un_out;

    // A frame size per sequence (gf_seq_size.hpp; gf_tracker_set_seq_size), the seventh thing addressed by SEQUENCE.  sizes: the sizes in force (row 0: the handle's
    // own) and each sequence's row, host memory only until a setter gives a sequence a size of its own.  Everything else is obtained by that first setter: d_size_rows,
    // the table as the kernels read it (a row written by the setter that takes it), and per call, by list position: the byte that names each position's row
    // (h_size_of: page-locked, carried to d_size_of by the copy list in front of LK and of the detection) and the compact per-size tables of the front's launches
    // (SizeSub below), which those launches read over the bus as they read the list.  size_plan: of the call in progress, or of a setter.
    gfsize::Table sizes;
    bool size_any = false;
    gfsize::Plan size_plan;
    std::vector<int> size_bpp;            // scratch of plan_sizes: bytes per pixel of each listed sequence's format
    // of a call with sizes, per distinct size g of the plan: how many of its members are converted / equalised, and where its slots of d_cvt / d_eq begin (bytes)
    // and its entries of the dense table of equalisation sources and sets of LUTs (entries)
    int size_ncvt[GF_MAX_SEQ_SIZES] = {}, size_neq[GF_MAX_SEQ_SIZES] = {}, size_eq_first[GF_MAX_SEQ_SIZES] = {};
    size_t size_cvt_at[GF_MAX_SEQ_SIZES] = {}, size_eq_at[GF_MAX_SEQ_SIZES] = {};
    PyrGeom size_geom[GF_MAX_SEQ_SIZES];
    DevBuf<SizeRow> d_size_rows;
    DevBuf<uint8_t> d_size_of; PinBuf<uint8_t> h_size_of;
    DevBuf<uint8_t> d_size_sub; PinBuf<uint8_t> h_size_sub;

    // A depth registration per sequence (gf_depth_reg.hpp; gf_tracker_set_seq_depth_reg), the eighth thing addressed by SEQUENCE.  Everything here is obtained by
    // the first setter of the handle: dreg_on[seq] / dreg[seq], the registration as it was set; d_dreg, [B] registered frames of cfg.width x cfg.height counts, a
    // sequence's frame written at its colour size in force, rows tight; dreg_stage, the z-buffer ([B] slots by list position) and the table of a call's jobs;
    // ev_dreg around the two kernels of a call, read when the stream is drained.
    std::vector<uint8_t> dreg_on; std::vector<gf_depth_reg> dreg;
    DevBuf<uint16_t> d_dreg;
    DepthRegStage dreg_stage;
    Event ev_dreg[2];
    long long dreg_launches = 0, dreg_frames = 0; double dreg_ms = 0;

    // rejectWithF per sequence (gf_reject_f.hpp; gf_tracker_set_seq_reject_f), the ninth thing addressed by SEQUENCE.  Everything here is obtained by the first
    // setter of the handle that turns a sequence's switch on: rf_on[seq] / rf[seq], the configuration as it was set; rf_stage, the table of a call's jobs and of
    // their results ([B] by job); ev_rf around the kernel of a call's first launch and of its second (a predicted sequence that fell back), read when the stream
    // is drained.  rf_host (GF_REJECT_F_HOST=1): gfrf::reject inside after_lk instead, no launch.
    std::vector<uint8_t> rf_on; std::vector<gf_reject_f_cfg> rf;
    RejectFStage rf_stage;
    Event ev_rf[4];
    bool rf_host = false;
    gf_reject_f_stats rf_stats{};

    // A right camera per sequence (gf_tracker_set_seq_stereo; the stereo branch of trackImage, feature_tracker.cpp:259-303; gf_stereo_kernels.hpp), the tenth thing
    // addressed by SEQUENCE.  Everything here is obtained by the first setter of the handle that turns a sequence's switch on: st_on[seq] / st_cfg[seq] / st_cam[seq],
    // the configuration as it was set and the right camera as the lift reads it; d_rimg, one right pyramid per sequence, the handle's slots apart; the table of
    // sizes where no size setter got it (the kernel reads a SizeRow per block).  Per call, by list position: st_right_of (the sequence, whose right pyramid the
    // call built, or -1), st_left_of (the call's cur_of), st_size_of, st_fb, st_ntr / st_row (the tracked survivors in final order as rows of LK's table, uploaded
    // with setMask's hand-over), and the kernel's outputs st_pts / st_status, which come up with the call's last copies.  st_refs / st_cur: the right frames and
    // their pyramids in the compact order of the pyramid launches (one per distinct size of the call).
    std::vector<uint8_t> st_on; std::vector<gf_stereo_cfg> st_cfg; std::vector<gfcam::Camera> st_cam;
    DevBuf<uint8_t> d_rimg;
    DevBuf<int> d_st_right_of, d_st_left_of, d_st_ntr, d_st_row, d_st_cur; PinBuf<int> h_st_right_of, h_st_left_of, h_st_ntr, h_st_row, h_st_cur;
    DevBuf<uint8_t> d_st_size_of, d_st_fb, d_st_status, d_st_fwd; PinBuf<uint8_t> h_st_size_of, h_st_fb, h_st_status;
    DevBuf<float2> d_st_pts; PinBuf<float2> h_st_pts;
    DevBuf<gf_frame_ref> d_st_refs; PinBuf<gf_frame_ref> h_st_refs;
    // the right cameras by sequence as the lift kernel reads them (a row written by the setter), the list of a call's right lifts on the device (the sequence, or -1:
    // a PINHOLE right camera, lifted on the host as a pinhole ever is, or a model GF_CAMERA_LIFT_HOST keeps there), the counts the stereo kernel leaves for the lift,
    // and the lifted pairs by position in cur_pts, which come up with the right points
    DevBuf<gfcam::Camera> d_st_cams; DevBuf<int> d_st_cam_of, d_st_n; PinBuf<int> h_st_cam_of;
    DevBuf<float2> d_st_un; PinBuf<float2> h_st_un;
    bool right_lifts_on_device(int q) const {   // the route the model takes today (lifts_on_device)
        const int m = st_cfg[q].right.model;
        if (m == GF_CAMERA_PINHOLE) return false;
        return lift_mode < 0 ? m != GF_CAMERA_SCARAMUZZA : lift_mode == 0;
    }
    // the right eye's CLAHE (the node equalises both eyes, rosNodeTest.cpp:256-261), obtained by the first setter that makes a stereo sequence an equalising one:
    // the equalised right frames the pyramid reads, their LUTs, and the dense table of a call's sources
    DevBuf<uint8_t> d_st_eq, d_st_eq_lut; DevBuf<gf_frame_ref> d_st_eqsrc; PinBuf<gf_frame_ref> h_st_eqsrc;
    gf_stereo_stats st_stats{};
    bool stereo_on(int q) const { return !st_on.empty() && st_on[q]; }

    // The depth a stereo sequence's matches determine (gf_tracker_set_seq_stereo_depth; gf_stereo_depth.hpp), the eleventh thing addressed by SEQUENCE.  Everything
    // here is obtained by the first setter of the handle that turns a switch on: sd_on[seq] / sd_cfg[seq], the configuration as it was set; d_sd_entries, by
    // SEQUENCE, what stereo_depth_kernel reads for a position through the stereo stage's own list (st_right_of names the sequence): both cameras, the rig and the
    // gates, on == 0 for a sequence without the switch; sd_entry, page-locked, what each row held when it last went down (gfsd::Entry has no padding, so equal bytes
    // are equal entries; a camera set after this setter makes the row go down
    // again, with the call that first finds it changed).  Per call, by list position: the kernel's outputs sd_mm / sd_why, which come up with the right points.
    // sd_host (GF_STEREO_DEPTH_HOST=1): gfsd::depth_of inside stereo_stage instead, no launch.
    std::vector<uint8_t> sd_on; std::vector<gf_stereo_depth_cfg> sd_cfg;
    DevBuf<gfsd::Entry> d_sd_entries; PinBuf<gfsd::Entry> sd_entry;
    DevBuf<uint16_t> d_sd_mm; PinBuf<uint16_t> h_sd_mm;
    DevBuf<uint8_t> d_sd_why; PinBuf<uint8_t> h_sd_why;
    bool sd_host = false;
    gf_stereo_depth_stats sd_stats{};
    bool stereo_depth_on(int q) const { return !sd_on.empty() && sd_on[q]; }

    std::unique_ptr<HostPool> pool;
};
static_assert(gfsize::kPad == gf::kPad && gfsize::kWin == gf::kWin && gfsize::kMaxLevels == gf::kMaxLevels, "gf_seq_size.hpp restates the pyramid's constants");
static_assert(sizeof(gfsize::Geom) == sizeof(gf::PyrGeom) && offsetof(gfsize::Geom, nlevels) == offsetof(gf::PyrGeom, nlevels) && offsetof(gfsize::Geom, img_bytes) == offsetof(gf::PyrGeom, img_bytes) &&
              sizeof(gfsize::Level) == sizeof(gf::LevelGeom) && offsetof(gfsize::Level, img_off) == offsetof(gf::LevelGeom, img_off), "gfsize::Geom is PyrGeom field for field");

namespace gf {

// buildOpticalFlowPyramid in three launches: level 0 (copy + REFLECT_101 border), level 1 (interior + border in one pass), and one kernel for
// all remaining levels.  There is no derivative pyramid: lk_solve evaluates the Scharr derivative of the template window itself.
// d_raw_frames: `count` frames back to back, frame i for the sequence at list position i; cur_of[i]: the pyramid it is written to (device-readable, [count]).
// refs (the _refs entry points, MONO8 without equalisation): the frames lie at refs[i] instead (device-readable table; d_raw_frames is not read).  The kernel
// follows the sizes as before and each block takes the load form its own frame's pointer and pitch allow.  *widest: the widest piece of the launched first reader.
// geom (a frame size per sequence, gf_seq_size.hpp): the geometry of the `count` frames where it is not the handle's; the pyramids still lie the handle's slots apart.
static int launch_pyramid(gf_tracker* h, const uint8_t* d_raw_frames, int count, const int* cur_of, const gf_frame_ref* refs = nullptr, int* widest = nullptr, const PyrGeom* geom = nullptr,
                          uint8_t* img_base = nullptr) {   // img_base: the pyramids cur_of counts in, where they are not the handle's pairs (the right pyramids of the stereo branch)
    const PyrGeom& G = geom ? *geom : h->G;
    const size_t seq_img = h->G.img_bytes;   // distance between two pyramids, whichever sequence and slot they belong to
    uint8_t* img = img_base ? img_base : h->d_img.p;
    const LevelGeom g0 = G.lv[0];
    const bool v16 = !((g0.w | g0.stride | (int)(((size_t)g0.w * g0.h) & 15) | (int)(seq_img & 15) | (int)((g0.img_off - kPad * g0.stride - kPad) & 15)) & 15) &&
                     !(((refs ? 0 : reinterpret_cast<uintptr_t>(d_raw_frames)) | reinterpret_cast<uintptr_t>(img)) & 15);
    bool vec = true;   // four-pixel kernels need level widths (and with them strides, offsets) that are multiples of 4
    for (int l = 0; l < G.nlevels; l++) vec = vec && !(G.lv[l].w & 3) && !(G.lv[l].img_off & 3);
    for (int l = 1; l < G.nlevels; l++) vec = vec && G.lv[l].w > kPad + 1 && G.lv[l].h > kPad + 1;   // one reflection reaches every border pixel
    // levels 0 and 1 from one read of the raw frame (pyr_head_kernel) when the sizes allow it; GF_PYR_HEAD=0 keeps the two kernels (A/B and fallback)
    const bool head = h->pyr_head && v16 && vec && G.nlevels >= 2 && !(g0.h & 1) && G.lv[1].h * 2 == g0.h && G.lv[1].w * 2 == g0.w && g0.h > kPad + 2 && g0.w > kPad + 2 &&
                      pyr_head_lds_bytes(g0.w) <= 64 * 1024;
    gf_tracker_stats& st = h->stats;
    if (head) {
        st.pyr_head++;
        const dim3 grid((G.lv[1].h + kHeadRows - 1) / kHeadRows, count);
        if (refs) pyr_head_refs_kernel<<<grid, 512, pyr_head_lds_bytes(g0.w), h->stream>>>(refs, img, seq_img, cur_of, g0, G.lv[1]);
        else pyr_head_kernel<<<grid, 512, pyr_head_lds_bytes(g0.w), h->stream>>>(d_raw_frames, (size_t)g0.w * g0.h, g0.w, img, seq_img, cur_of, g0, G.lv[1]);
    } else if (v16) {
        st.pyr_level0_vec16++;
        const int n = ((g0.w + 2 * kPad) / 16) * (g0.h + 2 * kPad);
        if (refs) pyr_level0_vec16_refs_kernel<<<dim3((n + 255) / 256, count), 256, 0, h->stream>>>(refs, img, seq_img, cur_of, g0);
        else pyr_level0_vec16_kernel<<<dim3((n + 255) / 256, count), 256, 0, h->stream>>>(d_raw_frames, (size_t)g0.w * g0.h, g0.w, img, seq_img, cur_of, g0);
    } else {
        st.pyr_level0_dword++;
        const int n = ((g0.w + 2 * kPad) / 4) * (g0.h + 2 * kPad);
        if (refs) pyr_level0_refs_kernel<<<dim3((n + 255) / 256, count), 256, 0, h->stream>>>(refs, img, seq_img, cur_of, g0);
        else pyr_level0_kernel<<<dim3((n + 255) / 256, count), 256, 0, h->stream>>>(d_raw_frames, (size_t)g0.w * g0.h, g0.w, img, seq_img, cur_of, g0);
    }
    if (widest) *widest = head || v16 ? 16 : 4;
    if (vec) {
        auto down = [&](int l) {
            const LevelGeom d = G.lv[l];
            st.pyr_down_pad4++;
            pyr_down_pad4_kernel<<<dim3(((d.w >> 2) * d.h + 255) / 256, count), 256, 0, h->stream>>>(img, seq_img, cur_of, G.lv[l - 1], d);
        };
        if (G.nlevels > 1 && !head) down(1);
        if (G.nlevels > 2) {
            const int parts = 4, last = std::min(G.nlevels - 1, 3);
            const LevelGeom d = G.lv[2], e = G.lv[last];
            const int band = last > 2 ? (e.h + parts - 1) / parts + 1 : ((d.h + 1) / 2 + parts - 1) / parts + 1;
            const size_t lds = (size_t)(2 * band + 4) * d.w + (last > 2 ? (size_t)band * e.w : 0);
            if (G.nlevels <= 4 && lds <= 64 * 1024) { st.pyr_down_tail++; pyr_down_tail_kernel<<<dim3(parts, count), 512, lds, h->stream>>>(img, seq_img, cur_of, G, 2); }
            else for (int l = 2; l < G.nlevels; l++) down(l);
        }
    } else {
        for (int l = 1; l < G.nlevels; l++) {
            const LevelGeom d = G.lv[l];
            const int n = (d.w + 2 * kPad) * (d.h + 2 * kPad);
            st.pyr_down_bytes++;
            pyr_down_kernel<<<dim3((n + 255) / 256, count), 256, 0, h->stream>>>(img, seq_img, cur_of, G.lv[l - 1], d);
        }
    }
    HIPCHK(hipGetLastError());
    return GF_OK;
}

// the one-shot building blocks at the end of the file: one frame into pyramid `slot` (0 or 1) of their batch-1 handle; d_cur[0] names it for the kernels that follow
static int launch_pyramid_one(gf_tracker* h, const uint8_t* d_raw_frame, int slot) {
    HIPCHK(hipStreamSynchronize(h->stream));   // h_cur may still be read by an earlier launch of the same helper
    h->h_cur.p[0] = slot;
    HIPCHK(hipMemcpyAsync(h->d_cur.p, h->h_cur.p, sizeof(int), hipMemcpyHostToDevice, h->stream));
    return launch_pyramid(h, d_raw_frame, 1, h->d_cur.p);
}

// One LK launch over the `batch` listed sequences in the form the handle was created for (same results in every form).
// REFS: A.depth is the call's table of gf_frame_ref (the _refs entry points with depth), read by the _refs forms of the same kernels.
template <bool REFS> static void launch_lk_form(gf_tracker* h, int batch, const LkBatchArgs& A) {
    const int cap = h->cap;
    if (h->lk_points == 4) (REFS ? lk_track_mp_refs_kernel<4> : lk_track_mp_kernel<4>)<<<dim3((cap + 15) / 16, batch), 256, 0, h->stream>>>(h->G, A);
    else if (h->lk_points == 2) (REFS ? lk_track_mp_refs_kernel<2> : lk_track_mp_kernel<2>)<<<dim3((cap + 7) / 8, batch), 256, 0, h->stream>>>(h->G, A);
    else (REFS ? lk_track_refs_kernel : lk_track_kernel)<<<dim3((cap + 3) / 4, batch), 256, 0, h->stream>>>(h->G, A);
}
// sized (a frame size per sequence): the forms that read each list position's geometry from the handle's table of sizes; A.depth is the call's table then
static void launch_lk_sized(gf_tracker* h, int batch, const LkBatchArgs& A) {
    const int cap = h->cap;
    const SizeRow* rows = h->d_size_rows.p; const uint8_t* of = h->d_size_of.p; const size_t slot = h->G.img_bytes;
    if (h->lk_points == 4) lk_track_mp_sized_kernel<4><<<dim3((cap + 15) / 16, batch), 256, 0, h->stream>>>(rows, of, slot, A);
    else if (h->lk_points == 2) lk_track_mp_sized_kernel<2><<<dim3((cap + 7) / 8, batch), 256, 0, h->stream>>>(rows, of, slot, A);
    else lk_track_sized_kernel<<<dim3((cap + 3) / 4, batch), 256, 0, h->stream>>>(rows, of, slot, A);
}
static void launch_lk(gf_tracker* h, int batch, const LkBatchArgs& A, bool depth_refs = false, bool sized = false) {
    if (sized) launch_lk_sized(h, batch, A); else if (depth_refs) launch_lk_form<true>(h, batch, A); else launch_lk_form<false>(h, batch, A);
}

static LkBatchArgs lk_args(gf_tracker* h, int fwd_max_level, int use_init, int flow_back, int post_checks, const uint8_t* seqmask,
                           const uint16_t* d_depth) {
    LkBatchArgs A{};
    A.img = h->d_img.p; A.cur_of = h->d_cur.p; A.cap = h->cap;
    A.n_pts = h->d_npts.p; A.prev_pts = h->d_prev_pts.p; A.init_pts = h->d_init_pts.p; A.cur_pts = h->d_cur_pts.p;
    A.status = h->d_status.p; A.fwd_status = h->d_fwd_status.p; A.depth_out = h->d_depth_out.p; A.depth = d_depth;
    A.depth_seq_stride = (size_t)h->cfg.width * h->cfg.height; A.depth_stride = h->cfg.width;
    A.counters = h->d_counters.p; A.fwd_max_level = fwd_max_level; A.fwd_use_init = use_init; A.flow_back = flow_back;
    A.post_checks = post_checks; A.seq_mask = seqmask;
    A.flow_back_of = h->d_seq_fb.p;   // null on a handle no setter has touched; written by the copy list in front of the call's first LK launch
    return A;
}

// The list of a call: `count` distinct sequences of the handle, in any order.  Checked before anything is copied, launched or changed.
static int check_list(gf_tracker* h, int count, const int* seq) {
    if (count < 0 || count > h->B) return set_err(GF_ERR_INVALID, "%d sequences listed for a handle of %d", count, h->B);
    if (count > 0 && !seq) return set_err(GF_ERR_INVALID, "null sequence list");
    h->listed.assign(h->B, 0);
    for (int i = 0; i < count; i++) {
        if (seq[i] < 0 || seq[i] >= h->B) return set_err(GF_ERR_INVALID, "list entry %d names sequence %d of a handle of %d", i, seq[i], h->B);
        if (h->listed[seq[i]]) return set_err(GF_ERR_INVALID, "sequence %d is listed twice", seq[i]);
        h->listed[seq[i]] = 1;
    }
    return GF_OK;
}

// The entry points that do not serve a depth registration (gf_tracker_set_seq_depth_reg; everything but the _refs forms): a call with depth that lists a
// sequence which has one is refused before anything is copied, launched or changed.  seq: checked by check_list.
static int refuse_registered(const gf_tracker* h, const char* who, int count, const int* seq, bool with_depth) {
    if (with_depth && !h->st_on.empty())   // the stereo branch likewise: the second image of a stereo sequence is its right frame, which travels by gf_frame_ref only
        for (int i = 0; i < count; i++)
            if (h->st_on[seq[i]])
                return set_err(GF_ERR_INVALID, "%s: sequence %d (list position %d) is a stereo sequence, which takes its right frame on gf_tracker_track_some_device_refs / "
                               "gf_tracker_track_batch_device_refs only; this entry point serves it without a second image, as a mono frame", who, seq[i], i);
    if (!with_depth || h->dreg_on.empty()) return GF_OK;
    for (int i = 0; i < count; i++)
        if (h->dreg_on[seq[i]])
            return set_err(GF_ERR_INVALID, "%s: sequence %d (list position %d) has a depth registration, which takes its raw depth frame on gf_tracker_track_some_device_refs / "
                           "gf_tracker_track_batch_device_refs only; this entry point serves it without depth", who, seq[i], i);
    return GF_OK;
}

// A frame size per sequence (gf_seq_size.hpp): whether the sequence has one of its own, and the frame everything of the sequence that is an image has.
static bool seq_has_size(const gf_tracker* h, int seq) { return h->size_any && h->sizes.row_of[seq] != 0; }
static int seq_width(const gf_tracker* h, int seq) { return h->sizes.w[h->sizes.row_of[seq]]; }     // the sequence's own frame, the handle's unless a setter said otherwise
static int seq_height(const gf_tracker* h, int seq) { return h->sizes.h[h->sizes.row_of[seq]]; }
static bool any_has_size(const gf_tracker* h, int count, const int* seq) { for (int i = 0; i < count; i++) if (seq_has_size(h, seq[i])) return true; return false; }

// ---- region of interest (gf_roi.hpp).  The setters run between frames: every track call returns with the handle's stream drained, so the table is never written
// under a detector that reads it; they leave on the same stream, in front of the next frame's kernels.
static int roi_ready(gf_tracker* h) {   // the first setter of a handle: the table, all-ones (no sequence has a region yet), and its host copy
    if (h->d_roi.p) return GF_OK;
    const size_t words = gfroi::words(h->cfg.width, h->cfg.height), all = (size_t)h->B * words;
    DevBuf<uint32_t> table; DevBuf<int> list;
    HIPCHK(table.alloc(all)); HIPCHK(list.alloc(h->B));
    HIPCHK(hipMemset(table.p, 0xff, all * sizeof(uint32_t)));
    HIPCHK(hipStreamSynchronize(nullptr));
    h->roi_bits.assign(all, ~0u); h->roi_has.assign(h->B, 0);
    h->roi_words = words;
    h->d_roi = std::move(table); h->d_roi_seq = std::move(list);
    return GF_OK;
}
static void roi_clear_host(gf_tracker* h, int seq) {
    std::fill_n(h->roi_bits.begin() + (size_t)seq * h->roi_words, h->roi_words, ~0u);
    h->roi_has[seq] = 0;
}
// the table the setters of R write: the detector's own until the handle has boxes, the base table from then on
static uint32_t* roi_base_table(gf_tracker* h) { return h->d_roi_base.p ? h->d_roi_base.p : h->d_roi.p; }
static int boxes_compose(gf_tracker* h, int count, const int* seq);
static int roi_packed(gf_tracker* h, int count, const int* seq) {   // behind a packing kernel: the words come back (setMask's walk reads them on the host) and the sequences have a region
    for (int i = 0; i < count; i++) {
        const size_t off = (size_t)seq[i] * h->roi_words;
        HIPCHK(hipMemcpyAsync(h->roi_bits.data() + off, roi_base_table(h) + off, h->roi_words * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < count; i++) h->roi_has[seq[i]] = 1;
    return h->d_roi_base.p ? boxes_compose(h, count, seq) : GF_OK;   // a new base under the boxes in force
}
// The device setters on a list with sizes (h->size_plan is its plan, h_refs[0 .. count) its masks): one launch, every mask packed in its own geometry
static int roi_pack_sized(gf_tracker* h, int count, const int* seq) {
    const gfsize::Plan& p = h->size_plan;
    for (int i = 0; i < count; i++) {
        h->h_size_of.p[i] = p.row[i];
        if (p.row[i] != 0) {   // the words its own geometry does not reach stay all ones
            const size_t off = (size_t)seq[i] * h->roi_words;
            HIPCHK(hipMemsetAsync(roi_base_table(h) + off, 0xff, h->roi_words * sizeof(uint32_t), h->stream));
        }
    }
    HIPCHK(hipMemcpyAsync(h->d_refs.p, h->h_refs.p, (size_t)count * sizeof(gf_frame_ref), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_size_of.p, h->h_size_of.p, (size_t)count, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_roi_seq.p, seq, (size_t)count * sizeof(int), hipMemcpyHostToDevice, h->stream));
    roi_pack_sized_kernel<<<dim3((p.max_w + 255) / 256, gfroi::bands(p.max_h), count), 256, 0, h->stream>>>(h->d_refs.p, h->d_roi_seq.p, h->d_size_rows.p, h->d_size_of.p, roi_base_table(h), h->roi_words);
    HIPCHK(hipGetLastError());
    return roi_packed(h, count, seq);
}
static int roi_upload(gf_tracker* h, int seq) {   // the host copy of one sequence's words -> the table
    const size_t off = (size_t)seq * h->roi_words;
    HIPCHK(hipMemcpyAsync(roi_base_table(h) + off, h->roi_bits.data() + off, h->roi_words * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));   // roi_bits is pageable
    return h->d_roi_base.p ? boxes_compose(h, 1, &seq) : GF_OK;
}

// ---- exclusion boxes (gf_roi.hpp).  The first box setter of a handle: the base table, a copy of what the detector's table holds (no sequence has boxes yet), the
// staging of a setter's jobs and boxes, and the lists themselves.
static int boxes_ready(gf_tracker* h) {
    if (h->d_roi_base.p) return GF_OK;
    if (int rc = roi_ready(h)) return rc;
    const size_t all = (size_t)h->B * h->roi_words, stage = (size_t)h->B * (sizeof(RoiBoxJob) + (size_t)GF_MAX_BOXES_PER_SEQ * sizeof(gf_box));
    DevBuf<uint32_t> base; DevBuf<uint8_t> dst; PinBuf<uint8_t> hst;
    HIPCHK(base.fit(all)); HIPCHK(dst.alloc(stage)); HIPCHK(hst.alloc(stage));
    if (!h->ev_boxes.e) HIPCHK(hipEventCreateWithFlags(&h->ev_boxes.e, hipEventDisableTiming));
    HIPCHK(hipMemcpyAsync(base.p, h->d_roi.p, all * sizeof(uint32_t), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->d_draw_prims.p) {   // a handle that shows tracks already: its rows of primitives gain room for the boxes' frames, and every list goes down again
        const size_t row = gfdraw::list_capacity(h->cap) + (size_t)GF_MAX_BOXES_PER_SEQ;
        DevBuf<gfdraw::Prim> dp; PinBuf<gfdraw::Prim> hp;
        HIPCHK(dp.alloc((size_t)h->B * row)); HIPCHK(hp.alloc((size_t)h->B * row));
        h->d_draw_prims = std::move(dp); h->h_draw_prims = std::move(hp);
        for (auto& q : h->seq) q.draw_sent = false;
    }
    h->boxes.assign(h->B, std::vector<gf_box>());
    h->d_roi_base = std::move(base); h->d_box_stage = std::move(dst); h->h_box_stage = std::move(hst);
    return GF_OK;
}
// The words of R_eff of the `count` listed sequences (checked by the caller) from their base words and the lists in h->boxes: the jobs and boxes into the page-locked
// staging, one copy and one launch on the handle's stream, no wait for either.  Only a call that finds the staging of an earlier one still unread waits for that.
static int boxes_compose(gf_tracker* h, int count, const int* seq) {
    if (count == 0) return GF_OK;
    if (h->box_pending) HIPCHK(hipEventSynchronize(h->ev_boxes));
    RoiBoxJob* jobs = reinterpret_cast<RoiBoxJob*>(h->h_box_stage.p);
    gf_box* list = reinterpret_cast<gf_box*>(jobs + count);   // right behind the jobs of THIS call: one copy carries both
    int total = 0;
    for (int i = 0; i < count; i++) {
        const std::vector<gf_box>& b = h->boxes[seq[i]];
        jobs[i] = RoiBoxJob{seq[i], total, (int)b.size(), h->sizes.row_of[seq[i]]};   // .pad: the row of the sequence's size, read by the sized form alone
        if (!b.empty()) memcpy(list + total, b.data(), b.size() * sizeof(gf_box));
        total += (int)b.size();
    }
    const size_t bytes = (size_t)count * sizeof(RoiBoxJob) + (size_t)total * sizeof(gf_box);
    HIPCHK(hipMemcpyAsync(h->d_box_stage.p, h->h_box_stage.p, bytes, hipMemcpyHostToDevice, h->stream));
    const RoiBoxJob* d_jobs = reinterpret_cast<const RoiBoxJob*>(h->d_box_stage.p);
    const int W = h->cfg.width, H = h->cfg.height;
    if (any_has_size(h, count, seq))   // a frame size per sequence: each job clipped to and composed in its own frame (every size is inside the grid of the handle's)
        roi_boxes_sized_kernel<<<dim3((W + kRoiBoxSpan - 1) / kRoiBoxSpan, gfroi::bands(H), count), kRoiBoxPiece, 0, h->stream>>>(
            d_jobs, reinterpret_cast<const gf_box*>(d_jobs + count), h->d_size_rows.p, h->d_roi_base.p, h->d_roi.p, h->roi_words);
    else
        roi_boxes_kernel<<<dim3((W + kRoiBoxSpan - 1) / kRoiBoxSpan, gfroi::bands(H), count), kRoiBoxPiece, 0, h->stream>>>(
            d_jobs, reinterpret_cast<const gf_box*>(d_jobs + count), W, H, h->d_roi_base.p, h->d_roi.p, h->roi_words);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev_boxes, h->stream));
    h->box_pending = true;
    return GF_OK;
}
// The lists of a box setter, before anything is copied, launched or changed; the message names the list position.
static int check_box_lists(gf_tracker* h, int count, const int* seq, const int* first, const gf_box* boxes) {
    if (count < 0 || count > h->B) return set_err(GF_ERR_INVALID, "%d sequences listed for a handle of %d", count, h->B);
    if (count > 0 && !seq) return set_err(GF_ERR_INVALID, "null sequence list");
    h->listed.assign(h->B, 0);
    for (int i = 0; i < count; i++) {
        if (seq[i] < 0 || seq[i] >= h->B) return set_err(GF_ERR_INVALID, "list position %d names sequence %d of a handle of %d", i, seq[i], h->B);
        if (h->listed[seq[i]]) return set_err(GF_ERR_INVALID, "list position %d names sequence %d a second time", i, seq[i]);
        h->listed[seq[i]] = 1;
    }
    if (count == 0 || (!first && !boxes)) return GF_OK;
    if (!first) return set_err(GF_ERR_INVALID, "boxes without the table of offsets `first` (list position 0)");
    if (first[0] != 0) return set_err(GF_ERR_INVALID, "list position 0: first[0] is %d, not 0", first[0]);
    for (int i = 0; i < count; i++) {
        if (first[i + 1] < first[i]) return set_err(GF_ERR_INVALID, "list position %d (sequence %d): first decreases from %d to %d", i, seq[i], first[i], first[i + 1]);
        if (first[i + 1] - first[i] > GF_MAX_BOXES_PER_SEQ)
            return set_err(GF_ERR_INVALID, "list position %d (sequence %d): %d boxes > GF_MAX_BOXES_PER_SEQ = %d", i, seq[i], first[i + 1] - first[i], GF_MAX_BOXES_PER_SEQ);
        if (!boxes && first[i + 1] > first[i]) return set_err(GF_ERR_INVALID, "list position %d (sequence %d): %d boxes listed but `boxes` is null", i, seq[i], first[i + 1] - first[i]);
    }
    return GF_OK;
}

// The row step of host frames on a handle that takes colour or raw frames: refused before anything is copied.  (A MONO8 handle hands its stride to the copy as it always did.)
// ---- formats per sequence (gf_seq_format.hpp).  The plan of the list of a call on a handle that has any: formats, sizes, offsets and slots by list position.
static void plan_call(gf_tracker* h, int count, const int* seq) {
    gfseqfmt::plan_list(h->plan, h->fmt.data(), gfseqfmt::of_handle(h->cfg), count, seq, h->cfg.width, h->cfg.height);
}
// ---- a frame size per sequence (gf_seq_size.hpp).  The plan of the list of a call on a handle that has any: each frame with its own size and its own format's bytes.
static void plan_sizes(gf_tracker* h, int count, const int* seq) {
    h->size_bpp.resize(count);
    for (int i = 0; i < count; i++) h->size_bpp[i] = gfpix::channels(h->fmt[seq[i]].pixel_format);
    gfsize::plan_list(h->size_plan, h->sizes, count, seq, h->size_bpp.data());
}
// The compact tables of such a call in the page-locked block h_size_sub / d_size_sub, each [B], entry k for list position size_plan.member[k]: what the pyramid
// reads, what the conversion reads (data null: skipped) and in which format (-1: skipped), the dense table of what the equalisation reads, and the entries of cur_of.
struct SizeSub {
    gf_frame_ref* pyr; gf_frame_ref* cvt; gf_frame_ref* eq; int* cur; int* fmt;
    SizeSub(uint8_t* base, size_t B) : pyr(reinterpret_cast<gf_frame_ref*>(base)), cvt(pyr + B), eq(cvt + B), cur(reinterpret_cast<int*>(eq + B)), fmt(cur + B) {}
    static size_t bytes(size_t B) { return B * (3 * sizeof(gf_frame_ref) + 2 * sizeof(int)); }
};
// The row steps of the host frames of a list on such a handle: each sequence's own (host_stride) or the call's, against a row of its own format.
static int check_strides_listed(gf_tracker* h, int count, const int* seq, int stride) {
    for (int i = 0; i < count; i++) {
        const gf_tracker_seq_format& f = h->fmt[seq[i]];
        const long long eff = gfseqfmt::host_stride(f, stride);
        const size_t row = gfseqfmt::row_bytes(h->cfg.width, f.pixel_format);
        if (eff < 0 || (size_t)eff < row)
            return set_err(GF_ERR_INVALID, "gray frame at list position %d (sequence %d): a stride of %lld bytes is shorter than a row of %d pixels of %d bytes (pixel format %d)", i, seq[i], eff, h->cfg.width,
                           gfpix::channels(f.pixel_format), f.pixel_format);
    }
    return GF_OK;
}
// The host frames of the list into `raw` (d_raw or d_raw2) on `stream`: each as it lies, with its own row bytes, to the sum of the frames before it.
static int copy_host_frames(gf_tracker* h, int count, const int* seq, const uint8_t* const* gray, int stride, uint8_t* raw, hipStream_t stream) {
    plan_call(h, count, seq);
    const int W = h->cfg.width, H = h->cfg.height;
    for (int i = 0; i < count; i++) {
        const size_t row = gfseqfmt::row_bytes(W, h->plan.format[i]);
        HIPCHK(hipMemcpy2DAsync(raw + h->plan.offset[i], row, gray[i], (size_t)gfseqfmt::host_stride(h->fmt[seq[i]], stride), row, H, hipMemcpyHostToDevice, stream));
    }
    return GF_OK;
}

static int check_stride(gf_tracker* h, int stride) {
    if (h->cfg.pixel_format && (stride < 0 || (size_t)stride < (size_t)h->cfg.width * h->ch))
        return set_err(GF_ERR_INVALID, "a stride of %d bytes is shorter than a row of %d pixels of %d bytes (gf_tracker_cfg.pixel_format %d)", stride, h->cfg.width, h->ch, h->cfg.pixel_format);
    return GF_OK;
}
// The host frames of the `count` listed sequences (gf_tracker_track_some, gf_tracker_prefetch_some), refused before anything is copied.
// *have_depth: the call has depth images, one for every listed sequence with a depth camera.
// *sized: a listed sequence has a frame size of its own; h->size_plan is the plan of the list then, and the rows are checked against each sequence's own width
static int check_host_frames(gf_tracker* h, int count, const int* seq, const uint8_t* const* gray, int stride, const uint16_t* const* depth, int dstride, bool* have_depth, bool* sized) {
    *sized = false;
    if (h->size_any) { plan_sizes(h, count, seq); *sized = h->size_plan.sized; }
    if (!*sized) {
        if (int rc = h->fmt_any ? check_strides_listed(h, count, seq, stride) : check_stride(h, stride)) return rc;
    } else {
        for (int i = 0; i < count; i++) {   // each sequence's own row step (host_stride) or the call's, against a row of its own width and format
            const gf_tracker_seq_format& f = h->fmt[seq[i]];
            const long long eff = gfseqfmt::host_stride(f, stride);
            const int w = h->size_plan.w[i];
            if (eff < 0 || (size_t)eff < gfseqfmt::row_bytes(w, f.pixel_format))
                return set_err(GF_ERR_INVALID, "gray frame at list position %d (sequence %d): a stride of %lld bytes is shorter than a row of its %d pixels of %d bytes (pixel format %d)", i, seq[i], eff, w,
                               gfpix::channels(f.pixel_format), f.pixel_format);
        }
    }
    *have_depth = depth != nullptr;
    for (int i = 0; i < count; i++) {
        if (!gray[i]) return set_err(GF_ERR_INVALID, "null image for sequence %d", seq[i]);
        if (*have_depth && !depth[i] && h->par[seq[i]].depth_cam) *have_depth = false;
    }
    if (*sized && *have_depth)
        for (int i = 0; i < count; i++)
            if (depth[i] && dstride < h->size_plan.w[i])
                return set_err(GF_ERR_INVALID, "depth frame at list position %d (sequence %d): a stride of %d pixels is shorter than a row of its %d pixels", i, seq[i], dstride, h->size_plan.w[i]);
    return GF_OK;
}
// The host frames of a list with sizes into `raw` on `stream`: each with its own rows, tight, at the sum of the frames before it (h->size_plan)
static int copy_host_frames_sized(gf_tracker* h, int count, const int* seq, const uint8_t* const* gray, int stride, uint8_t* raw, hipStream_t stream) {
    const gfsize::Plan& p = h->size_plan;
    for (int i = 0; i < count; i++) {
        const gf_tracker_seq_format& f = h->fmt[seq[i]];
        const size_t row = gfseqfmt::row_bytes(p.w[i], f.pixel_format);
        HIPCHK(hipMemcpy2DAsync(raw + p.gray_off[i], row, gray[i], (size_t)gfseqfmt::host_stride(f, stride), row, (size_t)p.h[i], hipMemcpyHostToDevice, stream));
    }
    return GF_OK;
}

// The detector and the selection over `count` list positions as the tracker runs them: kept points as circle centres, no explicit mask, the handle's tables of
// regions, circles and min_dist where a setter has made them (null otherwise).  gf_good_features overrides what it sets differently.
static DetectArgs detect_args(gf_tracker* h) {
    DetectArgs D{};
    D.pyr = h->d_img.p; D.pyr_bytes = h->G.img_bytes; D.frame_of = h->d_det.p; D.g = h->G.lv[0];
    D.mask = nullptr; D.mask_seq_stride = 0; D.centers = h->d_centers.p; D.n_centers = h->d_ncenters.p; D.cap = h->cap;
    D.roi = h->d_roi.p; D.roi_seq_words = h->roi_words;   // null on a handle no setter has touched
    D.disk_of = h->d_seq_disk.p;                          // likewise
    D.maxkey = h->d_maxkey.p; D.cand = h->d_cand.p; D.cand_seq_stride = (size_t)h->cand_cap; D.cand_cap = h->cand_cap; D.cand_count = h->d_cand_count.p;
    return D;
}
static void launch_detect(gf_tracker* h, int count, const DetectArgs& D) {
    const int W = h->cfg.width, H = h->cfg.height;
    detect_strip_kernel<kDS_R><<<dim3((W + kDS_W - 1) / kDS_W, (H + kDS_R - 1) / kDS_R, count), 64, 0, h->stream>>>(D, h->disk);
}
// a frame size per sequence: one launch gridded for the largest listed frame (W x H), every strip with its own frame's geometry
static void launch_detect_sized(gf_tracker* h, int count, const DetectArgs& D, int W, int H) {
    detect_strip_sized_kernel<kDS_R><<<dim3((W + kDS_W - 1) / kDS_W, (H + kDS_R - 1) / kDS_R, count), 64, 0, h->stream>>>(D, h->disk, h->d_size_rows.p, h->d_size_of.p);
}
static SelectArgs select_args(gf_tracker* h, const uint16_t* depth, int skip_small) {   // depth: tight device frames, the call's table of gf_frame_ref (launch_select<true>) or null
    const int W = h->cfg.width, H = h->cfg.height;
    SelectArgs S{};
    S.cand = h->d_cand.p; S.cand_seq_stride = (size_t)h->cand_cap; S.cand_cap = h->cand_cap; S.cand_count = h->d_cand_count.p; S.maxkey = h->d_maxkey.p; S.want = h->d_want.p;
    S.w = W; S.h = H; S.min_dist = h->cfg.min_dist; S.min_dist_of = h->d_seq_md.p; S.out_cap = h->cap; S.sort_cap = h->sort_cap; S.out_pts = h->d_out_pts.p; S.out_depth = h->d_out_depth.p; S.out_n = h->d_out_n.p;
    S.depth = depth; S.depth_seq_stride = (size_t)W * H; S.depth_stride = W; S.skip_small = skip_small;
    return S;
}
// topk: one maximum per corner for the sequences that want a handful (select_topk_kernel); sort: the others, or all of them, through the sort
template <bool REFS> static void launch_select(gf_tracker* h, int count, const SelectArgs& S, bool topk, bool sort) {
    if (topk) (REFS ? select_topk_refs_kernel : select_topk_kernel)<<<dim3(count), 1024, 0, h->stream>>>(S);
    if (sort) (REFS ? select_corners_refs_kernel : select_corners_kernel)<<<dim3(count), 1024, h->select_lds, h->stream>>>(S);
}
static void launch_select_sized(gf_tracker* h, int count, const SelectArgs& S, bool topk, bool sort) {
    if (topk) select_topk_sized_kernel<<<dim3(count), 1024, 0, h->stream>>>(S, h->d_size_rows.p, h->d_size_of.p);
    if (sort) select_corners_sized_kernel<<<dim3(count), 1024, h->select_lds, h->stream>>>(S, h->d_size_rows.p, h->d_size_of.p);
}

// Where the frames of a call lie, one per list position, in one of three forms: tight device frames with or without tight device depth frames (device());
// tight device frames and the callers' depth images on the host (with_host_depth()); or wherever the caller's tables of gf_frame_ref say (by_refs()).
//
// host_depth: one pointer per listed sequence, rows of host_dstride pixels.  The reference reads ONE pixel of the depth image per feature (feature_tracker.cpp:360
// `rightImg.at<ushort>(round(y), round(x))`), and on the host-image entry points both the image and the feature coordinates are on the host anyway: sampling there
// keeps 614 KB per frame and sequence (two thirds of an RGB-D VGA frame) off the bus.  Device depth keeps the sample in the kernels.  Same pixel, same rounding
// (round half away from zero on the float coordinates), same u16.
//
// gray_refs / depth_refs (checked by the caller): the tables go into h_refs with the list and only the first kernel that reads a caller's frame -- conversion, CLAHE
// or the pyramid's level-0 reader, and the depth samples of LK and the selection -- addresses it through them; the tight forms build nothing and run the kernels of before.
struct FrameInput {
    const uint8_t* gray = nullptr;   // tight frames of the handle's format, never written
    const uint16_t* depth = nullptr;
    const uint16_t* const* host_depth = nullptr; int host_dstride = 0;
    const gf_frame_ref* gray_refs = nullptr; const gf_frame_ref* depth_refs = nullptr;
    static FrameInput device(const uint8_t* gray, const uint16_t* depth) { FrameInput f; f.gray = gray; f.depth = depth; return f; }
    static FrameInput with_host_depth(const uint8_t* gray, const uint16_t* const* depth, int dstride) { FrameInput f; f.gray = gray; f.host_depth = depth; f.host_dstride = dstride; return f; }
    static FrameInput by_refs(const gf_frame_ref* gray, const gf_frame_ref* depth) { FrameInput f; f.gray_refs = gray; f.depth_refs = depth; return f; }
    bool have_depth() const { return depth || host_depth || depth_refs; }
    bool depth_by_refs() const { return depth_refs != nullptr; }
    // the image the host samples for list position b; a sequence without a depth camera: its image is not read (its samples are never reported) and may be null
    const uint16_t* host_image(int b, const gf_tracker_seq_cfg& par) const { return host_depth && par.depth_cam ? host_depth[b] : nullptr; }
    // row b of a table of the kernels' depth samples, or null in the form whose samples the host takes itself
    const uint16_t* kernel_samples(const PinBuf<uint16_t>& table, int b, int cap) const { return host_depth ? nullptr : table.p + (size_t)b * cap; }
};

// The hand-overs between the host's bookkeeping and the kernels -- two to four small tables down before LK, five up behind it, three down before the detection, four
// up behind it -- as one copy-list kernel each (gf_copy_list.hpp) instead of one hipMemcpyAsync per table: sixteen submissions and copy latencies per frame become four.
// GF_TRACKER_COPIES=1 (lists off): the plain copies, each where it is added.
class HandOver {
  public:
    HandOver(bool lists, hipStream_t stream) : lists_(lists), stream_(stream) {}
    template <class D, class P> void down(D& dev, P& pin, size_t count) {   // host -> device
        const size_t bytes = count * sizeof(*pin.p);
        if (lists_) cl_.add(pin.hd, dev.p, 1, bytes, bytes); else if (err_ == hipSuccess) err_ = hipMemcpyAsync(dev.p, pin.p, bytes, hipMemcpyHostToDevice, stream_);
    }
    template <class P, class D> void up(P& pin, D& dev, size_t count) {     // device -> host
        const size_t bytes = count * sizeof(*pin.p);
        if (lists_) cl_.add(dev.p, pin.hd, 1, bytes, bytes); else if (err_ == hipSuccess) err_ = hipMemcpyAsync(pin.p, dev.p, bytes, hipMemcpyDeviceToHost, stream_);
    }
    int flush() {   // what was added since the last one leaves as one launch
        HIPCHK(err_);
        if (!lists_) return GF_OK;
        if (!cl_.ok) return set_err(GF_ERR_HIP, "copy list: a page-locked buffer is not mapped into the device's address space (GF_TRACKER_COPIES=1 selects plain copies)");
        HIPCHK(cl_.launch<1>(stream_));
        cl_ = gfcopy::Builder();
        return GF_OK;
    }
  private:
    gfcopy::Builder cl_;
    const bool lists_;
    const hipStream_t stream_;
    hipError_t err_ = hipSuccess;
};

// the rows of the hand-over tables as gf_track_host.hpp takes them
static_assert(sizeof(float2) == sizeof(P2f) && alignof(float2) >= alignof(P2f) && offsetof(float2, x) == offsetof(P2f, x) && offsetof(float2, y) == offsetof(P2f, y), "float2 rows are passed as P2f rows");
static_assert(sizeof(int2) == sizeof(P2i) && alignof(int2) >= alignof(P2i) && offsetof(int2, x) == offsetof(P2i, x) && offsetof(int2, y) == offsetof(P2i, y), "int2 rows are passed as P2i rows");
static P2f* row(const PinBuf<float2>& t, size_t b, int cap) { return reinterpret_cast<P2f*>(t.p + b * cap); }
static P2i* row(const PinBuf<int2>& t, size_t b, int cap) { return reinterpret_cast<P2i*>(t.p + b * cap); }

// One call of track_core: what its stages share.  N, seq: the list; every hand-over table of the handle is indexed by the position in it.
struct Call {
    gf_tracker* h; int N; const int* seq; FrameInput in;
    HandOver ho;
    std::chrono::steady_clock::time_point tp = std::chrono::steady_clock::now();
    const int* cur_of = nullptr;          // the list where the kernels ahead of the first copy list read it (publish): d_cur, or over the bus the page-locked table itself
    const gf_frame_ref* refs = nullptr;   // the frame table likewise; null: tight frames
    bool refs_down = false;               // its depth half is still wanted on the device: with the first copy list that leaves
    const uint16_t* kdepth = nullptr;     // what LK and the selection sample: tight device depth frames, the device table's depth half (depth_by_refs) or null
    bool any_prev = false, any_pred = false, any_plain = false, any_want = false;
    bool lift = false;                    // a listed sequence has a camera that is lifted on the device (run_detect, book_after_detect)
    int n_lift = 0;                       // how many of them
    bool mixed = false;                   // a listed sequence runs with a format or switch that is not the handle's own: the front goes through h->plan
    const uint8_t* mix = nullptr;         // the table of a mixed call where the front's kernels read it (h_mix over the bus, or d_mix)
    bool did_cvt = false, did_eq = false; // the call converted / equalised at least one listed sequence (read_profile)
    bool sized = false;                   // a listed sequence has a frame size that is not the handle's: the call goes through h->size_plan and the sized forms
    bool size_of_down = false;            // the bytes that name each position's size are still wanted on the device: with the first copy list that leaves
    const uint8_t* sub = nullptr;         // the compact per-size tables (SizeSub) where the front's launches read them: h_size_sub over the bus, or d_size_sub
    std::vector<int> rf_pos;              // list positions of the jobs of the call's launch of reject_f_kernel, in job order (launch_reject_f)
    std::vector<gfrf::Result> rf_res;     // by list position: what rejectWithF left for the sequence (winner -2: it did not run)
    int rf_launches = 0;                  // launches of reject_f_kernel in this call: 0, 1, or 2 when a predicted sequence fell back
    int n_reg = 0;                        // listed sequences whose raw depth frame this call registers (publish fills their jobs, launch_depth_reg runs them)
    int n_st_lift = 0;                    // how many of them have their right points lifted by the call's launch of camera_lift_kernel
    int n_stereo = 0;                     // listed stereo sequences that came with a right frame: the stage runs for them (publish, launch_right_pyramids, launch_stereo)
    int n_sd = 0;                         // how many of them carry the depth their matches determine (gf_tracker_set_seq_stereo_depth): launch_stereo_depth, stereo_up
    void lap(double& acc) { const auto n = std::chrono::steady_clock::now(); acc += std::chrono::duration<double, std::milli>(n - tp).count(); tp = n; }
    void add_refs() {
        if (refs_down) { ho.down(h->d_refs, h->h_refs, (size_t)2 * h->B); refs_down = false; }
        if (size_of_down) { ho.down(h->d_size_of, h->h_size_of, (size_t)N); size_of_down = false; }
    }
};

// The list has to be readable on the device before the pyramid, which is launched before the first copy list so that it runs under the host's table filling.
// No extra submission and no synchronisation: the pyramid kernels read the page-locked table itself (one scalar load per block, as the copy-list kernels read
// their sources), and the copy list in front of LK brings it to d_cur for that kernel, which is bound by instruction issue and should find it in the L2 (the
// detector gets its own form, h_det, with its other tables).  With plain copies (GF_TRACKER_COPIES=1) it is one more copy, in front of the pyramid.
// The frame table goes the same two ways; its depth half is wanted on the device by LK and the selection.
static int publish(Call& c) {
    gf_tracker* h = c.h;
    const FrameInput& in = c.in;
    c.kdepth = in.depth;
    if (in.gray_refs) {
        for (int i = 0; i < c.N; i++) { h->h_refs.p[i] = in.gray_refs[i]; h->h_refs.p[h->B + i] = in.depth_refs ? in.depth_refs[i] : gf_frame_ref{nullptr, 0}; }
        if (in.depth_refs) c.kdepth = reinterpret_cast<const uint16_t*>(h->d_refs.p + h->B);   // what the _refs forms of LK and the selection read in the place of tight frames
        // a right camera per sequence: the entry is the RIGHT frame, 8-bit.  It leaves the table the depth samples read (the sequence has no depth camera) and goes
        // to the stage's own, by list position until launch_right_pyramids orders it
        if (!h->st_on.empty())
            for (int i = 0; i < c.N; i++) {
                const int q = c.seq[i];
                h->h_st_right_of.p[i] = -1;
                if (!h->st_on[q]) continue;
                h->h_refs.p[h->B + i] = gf_frame_ref{nullptr, 0};
                if (in.depth_refs && in.depth_refs[i].data) { h->h_st_right_of.p[i] = q; c.n_stereo++; if (h->stereo_depth_on(q)) c.n_sd++; }
            }
        // a depth registration per sequence (gf_depth_reg.hpp): the entry is the RAW frame; the table names the handle's registered frame in its place, and the
        // job goes to launch_depth_reg.  A sequence without a depth camera is never registered (its entry is never sampled).
        if (in.depth_refs && !h->dreg_on.empty()) {
            const size_t slot = (size_t)h->cfg.width * h->cfg.height, zslot = gfdreg::zwords_of(h->cfg.width, h->cfg.height);
            for (int i = 0; i < c.N; i++) {
                const int q = c.seq[i];
                if (!h->dreg_on[q]) continue;
                if (!h->par[q].depth_cam || !in.depth_refs[i].data) { h->h_refs.p[h->B + i] = gf_frame_ref{nullptr, 0}; continue; }   // a raw frame is no frame of the colour size: nothing samples it
                const gf_tracker_seq_cfg& par = h->par[q];
                const bool full = !h->cam_on.empty() && h->cam_on[q];   // with a registration set: a PINHOLE_FULL camera (the two setters see to it)
                const double proj[4] = {par.fx, par.fy, par.cx, par.cy}, dist[4] = {par.k1, par.k2, par.p1, par.p2};
                gfdreg::Job& j = h->dreg_stage.h_jobs.p[c.n_reg++];
                j.src = static_cast<const uint8_t*>(in.depth_refs[i].data); j.src_pitch = in.depth_refs[i].pitch;
                j.wd = h->dreg[q].width; j.hd = h->dreg[q].height; j.wc = seq_width(h, q); j.hc = seq_height(h, q);
                j.dst = reinterpret_cast<uint8_t*>(h->d_dreg.p + (size_t)q * slot); j.dst_pitch = (size_t)j.wc * 2;
                j.zoff = (size_t)i * zslot;
                j.p = full ? gfdreg::params_of(h->dreg[q], h->cam_model[q].proj, h->cam_model[q].dist, h->cam_model[q].dist + 4) : gfdreg::params_of(h->dreg[q], proj, dist);
                h->h_refs.p[h->B + i] = gf_frame_ref{j.dst, j.dst_pitch};
            }
        }
    }
    const bool over_bus = h->copy_lists && h->h_cur.hd;
    if (!over_bus) HIPCHK(hipMemcpyAsync(h->d_cur.p, h->h_cur.p, (size_t)c.N * sizeof(int), hipMemcpyHostToDevice, h->stream));
    c.cur_of = over_bus ? h->h_cur.hd : h->d_cur.p;
    const bool refs_bus = in.gray_refs && over_bus && h->h_refs.hd;
    if (in.gray_refs && !refs_bus) HIPCHK(hipMemcpyAsync(h->d_refs.p, h->h_refs.p, (size_t)2 * h->B * sizeof(gf_frame_ref), hipMemcpyHostToDevice, h->stream));
    c.refs = !in.gray_refs ? nullptr : refs_bus ? h->h_refs.hd : h->d_refs.p;
    c.refs_down = refs_bus && in.depth_refs;
    if (c.mixed) {   // the plan's three tables of sources and the formats, the same way
        gfseqfmt::Plan& p = h->plan;
        const int W = h->cfg.width, H = h->cfg.height;
        h->plan_frames.resize(c.N);
        if (in.gray_refs) std::copy(in.gray_refs, in.gray_refs + c.N, h->plan_frames.begin());
        else gfseqfmt::tight_frames(p, in.gray, W, h->plan_frames.data());   // base + the sum of the frames before it, rows tight
        gfseqfmt::plan_sources(p, h->plan_frames.data(), h->d_cvt.p, h->d_eq.p, W, H);
        gf_frame_ref* t = reinterpret_cast<gf_frame_ref*>(h->h_mix.p);
        int* f = reinterpret_cast<int*>(t + 3 * (size_t)h->B);
        for (int i = 0; i < c.N; i++) { t[i] = p.cvt_src[i]; t[2 * (size_t)h->B + i] = p.pyr_src[i]; f[i] = p.cvt_format[i]; }
        for (int j = 0; j < p.n_eq; j++) t[h->B + j] = p.eq_src[j];
        const bool mix_bus = over_bus && h->h_mix.hd;
        if (!mix_bus) HIPCHK(hipMemcpyAsync(h->d_mix.p, h->h_mix.p, h->h_mix.n, hipMemcpyHostToDevice, h->stream));
        c.mix = mix_bus ? h->h_mix.hd : h->d_mix.p;
    }
    if (c.sized) {   // a frame size per sequence (gf_seq_size.hpp): every frame by pointer and pitch, whichever way the caller handed it in
        const gfsize::Plan& p = h->size_plan;
        const size_t B = (size_t)h->B;
        // the depth half of the frame table, which the sized forms of LK and the selection sample through: the caller's entries, or tight frames at the sum of those before
        const bool kd = in.depth || in.depth_refs;
        if (!in.gray_refs)
            for (int i = 0; i < c.N; i++)
                h->h_refs.p[B + i] = in.depth ? gf_frame_ref{reinterpret_cast<const uint8_t*>(in.depth) + p.depth_off[i], (size_t)p.w[i] * 2} : gf_frame_ref{nullptr, 0};
        c.kdepth = kd ? reinterpret_cast<const uint16_t*>(h->d_refs.p + B) : nullptr;
        // the compact tables: entry k belongs to list position member[k].  Per distinct size the members that are converted take the slots of d_cvt from that
        // size's first on, in list order, and those that are equalised the slots of d_eq and the sets of LUTs likewise; each stage reads what the one before it left.
        SizeSub t(h->h_size_sub.p, B);
        size_t cvt_at = 0, eq_at = 0;
        int eq_first = 0;
        for (int g = 0; g < p.n_groups; g++) {
            const size_t px = (size_t)h->sizes.w[p.group_row[g]] * h->sizes.h[p.group_row[g]];
            const size_t pitch = (size_t)h->sizes.w[p.group_row[g]];
            h->size_cvt_at[g] = cvt_at; h->size_eq_at[g] = eq_at; h->size_eq_first[g] = eq_first;
            int n_cvt = 0, n_eq = 0;
            for (int k = p.group_first[g]; k < p.group_first[g] + p.group_n[g]; k++) {
                const int i = p.member[k];
                const gf_tracker_seq_format& f = h->fmt[c.seq[i]];
                gf_frame_ref cur = in.gray_refs ? in.gray_refs[i] : gf_frame_ref{in.gray + p.gray_off[i], gfseqfmt::row_bytes(p.w[i], f.pixel_format)};
                t.cur[k] = h->h_cur.p[i];
                const bool conv = f.pixel_format != GF_PIX_MONO8;
                t.fmt[k] = conv ? f.pixel_format : -1;
                t.cvt[k] = conv ? cur : gf_frame_ref{nullptr, 0};
                if (conv) { cur = gf_frame_ref{h->d_cvt.p + cvt_at + (size_t)(k - p.group_first[g]) * px, pitch}; n_cvt++; }   // the slot is the entry's index in its size's launch
                if (f.equalize) { t.eq[eq_first + n_eq] = cur; cur = gf_frame_ref{h->d_eq.p + eq_at + (size_t)n_eq * px, pitch}; n_eq++; }
                t.pyr[k] = cur;
            }
            h->size_ncvt[g] = n_cvt; h->size_neq[g] = n_eq;
            if (n_cvt) cvt_at += (size_t)p.group_n[g] * px;
            eq_at += (size_t)n_eq * px; eq_first += n_eq;
        }
        for (int i = 0; i < c.N; i++) h->h_size_of.p[i] = p.row[i];
        const bool sub_bus = over_bus && h->h_size_sub.hd;
        if (!sub_bus) HIPCHK(hipMemcpyAsync(h->d_size_sub.p, h->h_size_sub.p, h->h_size_sub.n, hipMemcpyHostToDevice, h->stream));
        c.sub = sub_bus ? h->h_size_sub.hd : h->d_size_sub.p;
        // the bytes and the depth half go down with the list: by the copy list in front of LK / the detection, or by plain copies here
        const bool tables_bus = over_bus && h->h_size_of.hd && h->h_refs.hd;
        if (tables_bus) { c.size_of_down = true; c.refs_down = kd; }
        else {
            HIPCHK(hipMemcpyAsync(h->d_size_of.p, h->h_size_of.p, (size_t)c.N, hipMemcpyHostToDevice, h->stream));
            if (kd) HIPCHK(hipMemcpyAsync(h->d_refs.p, h->h_refs.p, 2 * B * sizeof(gf_frame_ref), hipMemcpyHostToDevice, h->stream));
            c.refs_down = false;
        }
    }
    return GF_OK;
}

// Conversion to MONO8, equalisation and the pyramid, each reading what the stage before it left; only the first of them reads the caller's frames.
static int launch_front(Call& c) {
    gf_tracker* h = c.h;
    const int N = c.N, W = h->cfg.width, H = h->cfg.height;
    const bool prof = h->profiling;
    const uint8_t* gray = c.in.gray;
    const gf_frame_ref* refs = c.refs;
    int refs_widest = 16, refs_narrow = -1;   // the widest piece of the first reader of the caller's frames; frames it counted itself
    if (prof) HIPCHK(hipEventRecord(h->ev[0], h->stream));
    if (c.sized) {   // a frame size per sequence: each stage once per distinct size of the call that needs it, over that size's members -- conversion, CLAHE, and
        // one pass of launch_pyramid with the route a handle of that size takes
        const gfsize::Plan& p = h->size_plan;
        const SizeSub t(const_cast<uint8_t*>(c.sub), (size_t)h->B), ht(h->h_size_sub.p, (size_t)h->B);
        for (int g = 0; g < p.n_groups; g++) {
            if (!h->size_ncvt[g]) continue;
            const int first = p.group_first[g], fw = h->sizes.w[p.group_row[g]], fh = h->sizes.h[p.group_row[g]];
            if (int rc = cvt_launch_mixed(t.cvt + first, t.fmt + first, ht.cvt + first, ht.fmt + first, h->d_cvt.p + h->size_cvt_at[g], p.group_n[g], fw, fh, h->stream)) return rc;
            c.did_cvt = true;
        }
        if (c.did_cvt && prof) HIPCHK(hipEventRecord(h->ev[8], h->stream));
        for (int g = 0; g < p.n_groups; g++) {
            if (!h->size_neq[g]) continue;
            const int fw = h->sizes.w[p.group_row[g]], fh = h->sizes.h[p.group_row[g]];
            if (int rc = clahe_launch_refs(t.eq + h->size_eq_first[g], h->d_eq.p + h->size_eq_at[g], h->d_eq_lut.p + clahe_lut_bytes(h->size_eq_first[g], kClaheTiles, kClaheTiles), h->size_neq[g], fw, fh,
                                           kClaheClip, kClaheTiles, kClaheTiles, h->stream)) return rc;
            c.did_eq = true;
        }
        if (c.did_eq && prof) HIPCHK(hipEventRecord(h->ev[7], h->stream));
        for (int g = 0; g < p.n_groups; g++) {
            int widest = 16;
            if (int rc = launch_pyramid(h, nullptr, p.group_n[g], t.cur + p.group_first[g], t.pyr + p.group_first[g], &widest, &h->size_geom[p.group_row[g]])) return rc;
            if (c.in.gray_refs)   // each frame against the widest piece of ITS first reader: the conversion's dwords, CLAHE's or the pyramid's 16 bytes
                for (int k = p.group_first[g]; k < p.group_first[g] + p.group_n[g]; k++) {
                    const int i = p.member[k];
                    const gf_tracker_seq_format& f = h->fmt[c.seq[i]];
                    const int first_reader = f.pixel_format != GF_PIX_MONO8 ? 4 : f.equalize ? ((p.w[i] & 15) ? 4 : 16) : widest;
                    h->stats.frames_unaligned += gfref::unaligned(reinterpret_cast<uintptr_t>(c.in.gray_refs[i].data), c.in.gray_refs[i].pitch, first_reader) ? 1 : 0;
                }
        }
        if (prof) HIPCHK(hipEventRecord(h->ev[1], h->stream));
        return GF_OK;
    }
    if (c.mixed) {   // formats per sequence (gf_seq_format.hpp): the same three stages through the plan's tables, each over the positions that need it
        const gfseqfmt::Plan& p = h->plan;
        const gf_frame_ref* t = reinterpret_cast<const gf_frame_ref*>(c.mix);
        const gf_frame_ref* ht = reinterpret_cast<const gf_frame_ref*>(h->h_mix.p);
        const size_t B = (size_t)h->B;
        if (p.n_cvt) {
            if (int rc = cvt_launch_mixed(t, reinterpret_cast<const int*>(t + 3 * B), ht, reinterpret_cast<const int*>(ht + 3 * B), h->d_cvt.p, N, W, H, h->stream)) return rc;
            c.did_cvt = true;
            if (prof) HIPCHK(hipEventRecord(h->ev[8], h->stream));
        }
        if (p.n_eq) {
            if (int rc = clahe_launch_refs(t + B, h->d_eq.p, h->d_eq_lut.p, p.n_eq, W, H, kClaheClip, kClaheTiles, kClaheTiles, h->stream)) return rc;
            c.did_eq = true;
            if (prof) HIPCHK(hipEventRecord(h->ev[7], h->stream));
        }
        if (int rc = launch_pyramid(h, nullptr, N, c.cur_of, t + 2 * B, &refs_widest)) return rc;
        if (prof) HIPCHK(hipEventRecord(h->ev[1], h->stream));
        if (c.in.gray_refs) {   // each frame against the widest piece of ITS first reader: the conversion's dwords, CLAHE's or the pyramid's 16 bytes
            for (int i = 0; i < N; i++) {
                const int widest = p.cvt_format[i] >= 0 ? 4 : p.eq_index[i] >= 0 ? ((W & 15) ? 4 : 16) : refs_widest;
                h->stats.frames_unaligned += gfref::unaligned(reinterpret_cast<uintptr_t>(c.in.gray_refs[i].data), c.in.gray_refs[i].pitch, widest) ? 1 : 0;
            }
        }
        return GF_OK;
    }
    c.did_cvt = h->cfg.pixel_format != 0; c.did_eq = h->cfg.equalize != 0;
    if (h->cfg.pixel_format) {   // rosNodeTest.cpp:238-254: toCvCopy(msg, MONO8) ahead of CLAHE and trackImage
        if (int rc = refs ? cvt_launch_refs(refs, h->h_refs.p, h->cfg.pixel_format, h->d_cvt.p, N, W, H, h->stream, &refs_narrow)
                          : cvt_launch(gray, (size_t)W * h->ch, h->cfg.pixel_format, h->d_cvt.p, N, W, H, h->stream)) return rc;
        gray = h->d_cvt.p; refs = nullptr;
        if (prof) HIPCHK(hipEventRecord(h->ev[8], h->stream));
    }
    if (h->cfg.equalize) {   // rosNodeTest.cpp:256-261: CLAHE on the gray frame before trackImage, into the handle's buffer (the caller's frames stay as they are); frames and LUTs by list position
        if (int rc = refs ? clahe_launch_refs(refs, h->d_eq.p, h->d_eq_lut.p, N, W, H, kClaheClip, kClaheTiles, kClaheTiles, h->stream)
                          : clahe_launch(gray, h->d_eq.p, h->d_eq_lut.p, N, W, H, kClaheClip, kClaheTiles, kClaheTiles, h->stream)) return rc;
        if (refs) refs_widest = (W & 15) ? 4 : 16;
        gray = h->d_eq.p; refs = nullptr;
        if (prof) HIPCHK(hipEventRecord(h->ev[7], h->stream));
    }
    if (int rc = launch_pyramid(h, gray, N, c.cur_of, refs, refs ? &refs_widest : nullptr)) return rc;
    if (prof) HIPCHK(hipEventRecord(h->ev[1], h->stream));
    if (c.in.gray_refs) {
        if (refs_narrow < 0) { refs_narrow = 0; for (int i = 0; i < N; i++) refs_narrow += gfref::unaligned(reinterpret_cast<uintptr_t>(c.in.gray_refs[i].data), c.in.gray_refs[i].pitch, refs_widest) ? 1 : 0; }
        h->stats.frames_unaligned += refs_narrow;
    }
    return GF_OK;
}

// The raw depth frames of the call's registered sequences to their colour cameras (gf_depth_reg.hip): two launches for all of them, behind the pyramid and ahead
// of LK, the first kernel that samples depth.
static int launch_depth_reg(Call& c) {
    gf_tracker* h = c.h;
    if (int rc = depth_reg_launch(h->dreg_stage, c.n_reg, h->stream, h->ev_dreg[0], h->ev_dreg[1])) return rc;
    h->dreg_launches += 2; h->dreg_frames += c.n_reg;
    return GF_OK;
}

// rejectWithF (feature_tracker.cpp:711-743; gf_reject_f.hpp) of the listed sequences whose switch is on, in ONE launch behind LK on the tracking stream: the kernel
// rewrites the status bytes LK left on the device before they come up, so the host reads what it was going to read anyway.  only (may be null): by list position,
// the sequences of the launch (the second one of a call: those that fell back to the three-level LK).  A sequence with fewer than 8 points has no job: nothing
// would happen to it.
static bool seq_rejects(const gf_tracker* h, int q) { return !h->rf_on.empty() && h->rf_on[q]; }
static gfcam::Camera reject_f_camera(const gf_tracker* h, int q) {   // the camera the sequence is lifted with: its own, or the pinhole of its parameters
    if (!h->cam_on.empty() && h->cam_on[q]) return h->cam[q];
    gfcam::Camera cam{}; char msg[320];
    (void)gfcam::prepare(gfcam::pinhole_of(h->par[q]), cam, msg, sizeof msg);   // checked when the parameters were set
    return cam;
}
static int launch_reject_f(Call& c, const uint8_t* only) {
    gf_tracker* h = c.h;
    if (h->rf_on.empty() || h->rf_host) return GF_OK;
    const int cap = h->cap;
    c.rf_pos.clear();
    for (int i = 0; i < c.N; i++) {
        const int q = c.seq[i], n = h->h_npts.p[i];
        if (!h->rf_on[q] || n < gfrf::kSample || (only && !only[i])) continue;
        const gfcam::Camera cam = reject_f_camera(h, q);
        const gf_reject_f_cfg& f = h->rf[q];
        reject_f_job(h->rf_stage, (int)c.rf_pos.size(), &cam, h->d_prev_pts.p + (size_t)i * cap, h->d_cur_pts.p + (size_t)i * cap, nullptr, h->d_status.p + (size_t)i * cap, n,
                     seq_width(h, q), seq_height(h, q), f.f_threshold, f.focal_length == 0.0 ? gfrf::kFocal : f.focal_length,
                     gfrf::frame_seed(f.seed, (uint32_t)h->seq[q].frames));
        c.rf_pos.push_back(i);
    }
    if (c.rf_pos.empty()) return GF_OK;
    const int k = 2 * c.rf_launches;
    if (int rc = reject_f_launch(h->rf_stage, (int)c.rf_pos.size(), h->stream, h->ev_rf[k], h->ev_rf[k + 1])) return rc;
    c.rf_launches++;
    h->rf_stats.launches++;
    return GF_OK;
}
// the results of the launch, once the host has waited for the stream
static void collect_reject_f(Call& c) {
    if (c.rf_pos.empty()) return;
    if (c.rf_res.empty()) c.rf_res.assign(c.N, gfrf::Result{0, 0, -2, 0});
    for (size_t k = 0; k < c.rf_pos.size(); k++) c.rf_res[c.rf_pos[k]] = c.h->rf_stage.h_res.p[k];
    c.rf_pos.clear();
}

static int stereo_lk_launch(const SizeRow* rows, const uint8_t* size_of, size_t slot_bytes, const StereoLkArgs& A, int count, hipStream_t stream);

// The right pyramids of the call's stereo sequences that came with a right frame (feature_tracker.cpp:273 builds them inside calcOpticalFlowPyrLK): behind the
// front, by the pyramid route a frame of that size takes, one pass of launch_pyramid per distinct size among them, into d_rimg (pyramid q of sequence q).
static int launch_right_pyramids(Call& c) {
    gf_tracker* h = c.h;
    const bool bus = h->copy_lists && h->h_st_cur.hd && h->h_st_refs.hd;
    int first[GF_MAX_SEQ_SIZES + 1] = {0}, k = 0;
    int eq_n[GF_MAX_SEQ_SIZES] = {0}, eq_first[GF_MAX_SEQ_SIZES] = {0}, n_eq = 0;
    size_t eq_at[GF_MAX_SEQ_SIZES] = {0}, eq_bytes = 0;
    for (int r = 0; r < GF_MAX_SEQ_SIZES; r++) {   // the compact tables, size by size
        first[r] = k;
        for (int i = 0; i < c.N; i++) {
            const int q = c.seq[i];
            if (h->h_st_right_of.p[i] < 0 || h->sizes.row_of[q] != r) continue;
            h->h_st_cur.p[k] = q; h->h_st_refs.p[k] = c.in.depth_refs[i];
            if (h->fmt[q].equalize) {   // the pyramid reads the equalised frame: slot n_eq of the dense table, tight rows of the sequence's own width
                const size_t px = (size_t)seq_width(h, q) * seq_height(h, q);
                if (eq_n[r] == 0) { eq_first[r] = n_eq; eq_at[r] = eq_bytes; }
                h->h_st_eqsrc.p[n_eq] = c.in.depth_refs[i];
                h->h_st_refs.p[k] = gf_frame_ref{h->d_st_eq.p + eq_bytes, (size_t)seq_width(h, q)};
                eq_n[r]++; n_eq++; eq_bytes += px;
            }
            k++;
        }
    }
    first[GF_MAX_SEQ_SIZES] = k;
    if (n_eq) {   // CLAHE over the list, once per distinct size, as the sized front runs it
        const bool ebus = h->copy_lists && h->h_st_eqsrc.hd;
        if (!ebus) HIPCHK(hipMemcpyAsync(h->d_st_eqsrc.p, h->h_st_eqsrc.p, (size_t)n_eq * sizeof(gf_frame_ref), hipMemcpyHostToDevice, h->stream));
        const gf_frame_ref* src = ebus ? h->h_st_eqsrc.hd : h->d_st_eqsrc.p;
        for (int r = 0; r < GF_MAX_SEQ_SIZES; r++) {
            if (!eq_n[r]) continue;
            if (int rc = clahe_launch_refs(src + eq_first[r], h->d_st_eq.p + eq_at[r], h->d_st_eq_lut.p + clahe_lut_bytes(eq_first[r], kClaheTiles, kClaheTiles), eq_n[r], h->sizes.w[r], h->sizes.h[r],
                                           kClaheClip, kClaheTiles, kClaheTiles, h->stream)) return rc;
        }
    }
    if (!bus) {
        HIPCHK(hipMemcpyAsync(h->d_st_cur.p, h->h_st_cur.p, (size_t)k * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_st_refs.p, h->h_st_refs.p, (size_t)k * sizeof(gf_frame_ref), hipMemcpyHostToDevice, h->stream));
    }
    const int* cur = bus ? h->h_st_cur.hd : h->d_st_cur.p;
    const gf_frame_ref* refs = bus ? h->h_st_refs.hd : h->d_st_refs.p;
    for (int r = 0; r < GF_MAX_SEQ_SIZES; r++) {
        const int n = first[r + 1] - first[r];
        if (n < 1) continue;
        if (int rc = launch_pyramid(h, nullptr, n, cur + first[r], refs + first[r], nullptr, r == 0 ? nullptr : &h->size_geom[r], h->d_rimg.p)) return rc;
    }
    h->st_stats.right_pyramids += k;
    return GF_OK;
}

// The stereo tables that go down with setMask's hand-over (the copy list in front of the detection, or one of their own), and the ONE launch of the stereo kernel
// for all stereo sequences of the call, behind the selection kernel whose output table and counts it reads.
static void stereo_down(Call& c) {
    gf_tracker* h = c.h;
    const int N = c.N;
    for (int i = 0; i < N; i++) {
        const int q = c.seq[i];
        h->h_st_left_of.p[i] = h->h_cur.p[i]; h->h_st_size_of.p[i] = (uint8_t)h->sizes.row_of[q]; h->h_st_fb.p[i] = (uint8_t)(h->par[q].flow_back ? 1 : 0);
        if (h->h_st_right_of.p[i] < 0) h->h_st_ntr.p[i] = 0;
        const bool dev = h->h_st_right_of.p[i] >= 0 && h->right_lifts_on_device(q);
        h->h_st_cam_of.p[i] = dev ? q : -1;
        if (dev) c.n_st_lift++;
    }
    if (c.n_st_lift) c.ho.down(h->d_st_cam_of, h->h_st_cam_of, N);
    c.ho.down(h->d_st_right_of, h->h_st_right_of, N); c.ho.down(h->d_st_left_of, h->h_st_left_of, N); c.ho.down(h->d_st_size_of, h->h_st_size_of, N);
    c.ho.down(h->d_st_fb, h->h_st_fb, N); c.ho.down(h->d_st_ntr, h->h_st_ntr, N); c.ho.down(h->d_st_row, h->h_st_row, (size_t)N * h->cap);
}
static int launch_stereo(Call& c) {
    gf_tracker* h = c.h;
    StereoLkArgs A{};
    A.left = h->d_img.p; A.left_of = h->d_st_left_of.p; A.right = h->d_rimg.p; A.right_of = h->d_st_right_of.p; A.cap = h->cap;
    A.n_tracked = h->d_st_ntr.p; A.row = h->d_st_row.p; A.lk_pts = h->d_cur_pts.p; A.n_new = h->d_out_n.p; A.new_pts = h->d_out_pts.p;
    A.flow_back_of = h->d_st_fb.p; A.right_pts = h->d_st_pts.p; A.status = h->d_st_status.p; A.fwd_status = h->d_st_fwd.p; A.n_points = h->d_st_n.p;
    if (int rc = stereo_lk_launch(h->d_size_rows.p, h->d_st_size_of.p, h->G.img_bytes, A, c.N, h->stream)) return rc;
    h->st_stats.launches++;
    return GF_OK;
}
// The depth the call's matches determine (gf_stereo_depth.hpp), for the listed stereo sequences whose switch is on: ONE launch of stereo_depth_kernel behind the
// stereo kernel, whose right points and status bytes it reads where that kernel left them and whose gather of the left points it repeats.  The positions are
// named by the stereo stage's own list (d_st_right_of: the sequence, or -1), so nothing more goes down with the call; a sequence's row of d_sd_entries goes down
// here only where a setter changed what it is made of since it last did (the sequence's first frame, as a rule).
static gfsd::Entry stereo_depth_entry(const gf_tracker* h, int q) {   // what the sequence's depths are made of, as things stand: its two cameras, the rig, the gates
    gfsd::Entry e{};
    e.left = reject_f_camera(h, q); e.right = h->st_cam[q]; e.rig = gfsd::rig_of(h->sd_cfg[q]); e.on = 1;
    return e;
}
static gfcam::Pair* pairs(float2* p);
static int launch_stereo_depth(Call& c) {
    gf_tracker* h = c.h;
    if (!c.n_sd || h->sd_host) return GF_OK;
    for (int i = 0; i < c.N; i++) {
        const int q = c.seq[i];
        if (h->h_st_right_of.p[i] < 0 || !h->sd_on[q]) continue;
        const gfsd::Entry e = stereo_depth_entry(h, q);
        if (memcmp(&e, h->sd_entry.p + q, sizeof e) == 0) continue;   // no padding in an Entry (gf_stereo_depth.hpp): the bytes are the value
        h->sd_entry.p[q] = e;
        HIPCHK(hipMemcpyAsync(h->d_sd_entries.p + q, h->sd_entry.p + q, sizeof e, hipMemcpyHostToDevice, h->stream));
    }
    gfsd::Args A{};
    A.entries = h->d_sd_entries.p; A.entry_of = h->d_st_right_of.p; A.first = nullptr; A.cap = h->cap; A.count = c.N;
    A.n_tracked = h->d_st_ntr.p; A.row = h->d_st_row.p; A.lk_pts = pairs(h->d_cur_pts.p); A.n_new = h->d_out_n.p; A.new_pts = pairs(h->d_out_pts.p);
    A.right_pts = pairs(h->d_st_pts.p); A.status = h->d_st_status.p; A.depth_mm = h->d_sd_mm.p; A.why = h->d_sd_why.p;
    if (int rc = stereo_depth_launch(A, h->cap, h->stream)) return rc;
    h->sd_stats.launches++;
    return GF_OK;
}
static void stereo_up(Call& c) {
    gf_tracker* h = c.h;
    c.ho.up(h->h_st_pts, h->d_st_pts, (size_t)c.N * h->cap);
    c.ho.up(h->h_st_status, h->d_st_status, (size_t)c.N * h->cap);
    if (c.n_sd && !h->sd_host) { c.ho.up(h->h_sd_mm, h->d_sd_mm, (size_t)c.N * h->cap); c.ho.up(h->h_sd_why, h->d_sd_why, (size_t)c.N * h->cap); }
    if (c.n_st_lift) c.ho.up(h->h_st_un, h->d_st_un, (size_t)c.N * h->cap);
}

// Temporal optical flow (feature_tracker.cpp:113-176): the sequences without a prediction in one launch from scratch, those with one in a second from their
// predictions.  Returns when LK's tables are on the host.
static int run_lk(Call& c) {
    gf_tracker* h = c.h;
    const int N = c.N, cap = h->cap;
    const int* seq = c.seq;
    HandOver& ho = c.ho;
    for (int i = 0; i < N; i++) {
        bool has = false, pred = false;
        char msg[256];
        if (int rc = stage_points(h->seq[seq[i]], seq[i], cap, row(h->h_prev_pts, i, cap), row(h->h_init_pts, i, cap), h->h_npts.p + i, &has, &pred, msg, sizeof msg)) return set_err(rc, "%s", msg);
        c.any_prev |= has; c.any_pred |= pred; c.any_plain |= has && !pred;
    }
    if (c.any_prev) {
        if (c.cur_of != h->d_cur.p) ho.down(h->d_cur, h->h_cur, N);   // read over the bus so far
        c.add_refs();
        ho.down(h->d_npts, h->h_npts, N);
        if (h->d_seq_fb.p) { for (int i = 0; i < N; i++) h->h_seq_fb.p[i] = (uint8_t)h->par[seq[i]].flow_back; ho.down(h->d_seq_fb, h->h_seq_fb, N); }
        ho.down(h->d_prev_pts, h->h_prev_pts, (size_t)N * cap);
        const uint8_t* mask_plain = nullptr; const uint8_t* mask_pred = nullptr;
        if (c.any_pred) {
            ho.down(h->d_init_pts, h->h_init_pts, (size_t)N * cap);
            for (int i = 0; i < N; i++) { const bool pred = h->seq[seq[i]].hasPrediction; h->h_seqmask.p[i] = pred ? 0 : 1; h->h_seqmask.p[N + i] = pred ? 1 : 0; }
            ho.down(h->d_seqmask, h->h_seqmask, 2 * (size_t)N);
            mask_plain = h->d_seqmask.p; mask_pred = h->d_seqmask.p + N;
        }
        if (int rc = ho.flush()) return rc;
        if (h->profiling) HIPCHK(hipEventRecord(h->ev[2], h->stream));
        if (c.any_plain) { launch_lk(h, N, lk_args(h, 3, 0, h->cfg.flow_back, 1, mask_plain, c.kdepth), c.in.depth_by_refs(), c.sized); h->stats.lk_launches++; }
        if (c.any_pred) { launch_lk(h, N, lk_args(h, 1, 1, h->cfg.flow_back, 1, mask_pred, c.kdepth), c.in.depth_by_refs(), c.sized); h->stats.lk_launches++; }
        HIPCHK(hipGetLastError());
        if (h->profiling) HIPCHK(hipEventRecord(h->ev[3], h->stream));
        if (int rc = launch_reject_f(c, nullptr)) return rc;
        ho.up(h->h_cur_pts, h->d_cur_pts, (size_t)N * cap);
        ho.up(h->h_status, h->d_status, (size_t)N * cap);
        ho.up(h->h_fwd_status, h->d_fwd_status, (size_t)N * cap);
        ho.up(h->h_depth_out, h->d_depth_out, (size_t)N * cap);
        ho.up(h->h_counters, h->d_counters, (size_t)N * cap * 2);
        if (int rc = ho.flush()) return rc;
    }
    HIPCHK(hipEventRecord(h->ev[6], h->stream));
    c.lap(h->stats.ms_host_pre);
    HIPCHK(hipEventSynchronize(h->ev[6]));
    collect_reject_f(c);
    c.lap(h->stats.ms_wait_lk);
    return GF_OK;
}

// feature_tracker.cpp:124-132: fewer than 10 forward successes -> redo with 3 levels from scratch (per listed sequence: its neighbours in the call keep their pass)
static int redo_fallback(Call& c) {
    gf_tracker* h = c.h;
    const int N = c.N, cap = h->cap;
    if (!c.any_pred) return GF_OK;
    bool need = false;
    for (int i = 0; i < N; i++) {
        h->h_seqmask.p[i] = prediction_failed(h->seq[c.seq[i]], h->h_fwd_status.p + (size_t)i * cap, h->h_npts.p[i]) ? 1 : 0;
        need |= h->h_seqmask.p[i] != 0;
    }
    if (!need) return GF_OK;
    std::vector<uint8_t> redo(h->h_seqmask.p, h->h_seqmask.p + N);
    std::vector<uint8_t> keep_status(h->h_status.p, h->h_status.p + (size_t)N * cap);
    std::vector<float2> keep_pts(h->h_cur_pts.p, h->h_cur_pts.p + (size_t)N * cap);
    std::vector<uint16_t> keep_depth(h->h_depth_out.p, h->h_depth_out.p + (size_t)N * cap);
    std::vector<unsigned> keep_cnt(h->h_counters.p, h->h_counters.p + (size_t)N * cap * 2);
    HIPCHK(hipMemcpyAsync(h->d_seqmask.p, h->h_seqmask.p, N, hipMemcpyHostToDevice, h->stream));
    launch_lk(h, N, lk_args(h, 3, 0, h->cfg.flow_back, 1, h->d_seqmask.p, c.kdepth), c.in.depth_by_refs(), c.sized);
    h->stats.lk_launches++;
    HIPCHK(hipGetLastError());
    if (int rc = launch_reject_f(c, redo.data())) return rc;   // the first launch judged statuses that this pass replaces
    c.ho.up(h->h_cur_pts, h->d_cur_pts, (size_t)N * cap);
    c.ho.up(h->h_status, h->d_status, (size_t)N * cap);
    c.ho.up(h->h_depth_out, h->d_depth_out, (size_t)N * cap);
    c.ho.up(h->h_counters, h->d_counters, (size_t)N * cap * 2);
    if (int rc = c.ho.flush()) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    collect_reject_f(c);
    for (int i = 0; i < N; i++) {
        unsigned* cn = h->h_counters.p + (size_t)i * cap * 2;
        const unsigned* kc = keep_cnt.data() + (size_t)i * cap * 2;
        if (redo[i]) { for (int k = 0; k < 2 * cap; k++) cn[k] += kc[k]; continue; }  // both passes did work
        memcpy(h->h_status.p + (size_t)i * cap, keep_status.data() + (size_t)i * cap, cap);
        memcpy(h->h_cur_pts.p + (size_t)i * cap, keep_pts.data() + (size_t)i * cap, cap * sizeof(float2));
        memcpy(h->h_depth_out.p + (size_t)i * cap, keep_depth.data() + (size_t)i * cap, cap * sizeof(uint16_t));
        memcpy(cn, kc, cap * 2 * sizeof(unsigned));
    }
    return GF_OK;
}

// Host bookkeeping behind LK (after_lk, gf_track_host.hpp) per listed sequence on the pool, and the detector's form of the list.
static void book_after_lk(Call& c) {
    gf_tracker* h = c.h;
    const int cap = h->cap;
    std::atomic<long long> a_levels{0}, a_iters{0}, a_points{0}, a_tracked{0};
    std::atomic<int> a_want{0};
    std::atomic<long long> a_rf_seq{0}, a_rf_cand{0}, a_rf_rej{0}, a_rf_void{0};
    h->pool->parallel_for(c.N, [&](int b) {   // b: list position
        const int q = c.seq[b];
        const gf_tracker_seq_cfg& par = h->par[q];
        const size_t at = (size_t)b * cap;
        const LkRows r{row(h->h_cur_pts, b, cap), h->h_status.p + at, c.in.kernel_samples(h->h_depth_out, b, cap), h->h_counters.p + 2 * at, c.in.host_image(b, par), c.in.host_dstride};
        const uint32_t* roi = !h->roi_has.empty() && h->roi_has[q] ? h->roi_bits.data() + (size_t)q * h->roi_words : nullptr;
        int want = 0;
        const gf_box* boxes = h->boxes.empty() ? nullptr : h->boxes[q].data();
        const int fw = c.sized ? h->size_plan.w[b] : h->cfg.width, fh = c.sized ? h->size_plan.h[b] : h->cfg.height;   // the sequence's own frame (feature_tracker.cpp:108-109)
        RejectFHost rf{};   // GF_REJECT_F_HOST=1: the stage runs inside after_lk, on the status bytes as they came up
        const bool rf_here = h->rf_host && seq_rejects(h, q);
        if (rf_here) {
            rf.cam = reject_f_camera(h, q); rf.status = h->h_status.p + at;
            rf.f_threshold = h->rf[q].f_threshold; rf.focal = h->rf[q].focal_length == 0.0 ? gfrf::kFocal : h->rf[q].focal_length;
            rf.seed = gfrf::frame_seed(h->rf[q].seed, (uint32_t)h->seq[q].frames);
        }
        const LkTally n = after_lk(h->seq[q], par, fw, fh, h->seq_disk.empty() ? h->disk : h->seq_disk[q], roi, r, row(h->h_centers, b, cap), h->h_ncenters.p + b, &want,
                                   boxes, boxes ? (int)h->boxes[q].size() : 0, h->lifts_on_device(q) || (c.n_stereo && h->h_st_right_of.p[b] >= 0), rf_here ? &rf : nullptr);
        if (c.n_stereo && h->h_st_right_of.p[b] >= 0) {   // the tracked survivors in setMask's order, as rows of LK's table: the stereo kernel's first source
            const SeqState& s = h->seq[q];
            int* rows = h->h_st_row.p + at;
            for (size_t k = 0; k < s.lk_row.size(); k++) rows[k] = s.lk_row[k];
            h->h_st_ntr.p[b] = (int)s.lk_row.size();
        }
        if (rf_here && rf.ran) { a_rf_seq++; a_rf_cand += rf.result.m; a_rf_rej += rf.result.rejected; if (rf.result.m >= gfrf::kSample && rf.result.winner < 0) a_rf_void++; }
        a_levels += n.level_passes; a_iters += n.iterations; a_points += n.points; a_tracked += n.tracked;
        h->h_want.p[b] = want;
        if (h->h_seq_md.p) h->h_seq_md.p[b] = par.min_dist;
        h->h_det.p[b] = want > 0 ? h->h_cur.p[b] : -1;
        if (want > 0) a_want = 1;
        h->h_out_n.p[b] = 0;
    });
    c.any_want = a_want.load() != 0;
    for (const gfrf::Result& r : c.rf_res)   // the device form: what the call's launches left, a sequence that fell back counted once
        if (r.winner != -2) { a_rf_seq++; a_rf_cand += r.m; a_rf_rej += r.rejected; if (r.m >= gfrf::kSample && r.winner < 0) a_rf_void++; }
    h->rf_stats.sequences += a_rf_seq; h->rf_stats.candidates += a_rf_cand; h->rf_stats.rejected += a_rf_rej; h->rf_stats.no_model += a_rf_void;
    if (h->d_cams.p)   // a sequence lifted on the host is not listed: the kernel skips it, and a call that lists none has no launch
        for (int b = 0; b < c.N; b++) { const int q = c.seq[b]; const bool dev = h->lifts_on_device(q); h->h_cam_of.p[b] = dev ? q : -1; c.lift |= dev; if (dev) c.n_lift++; }
    h->stats.lk_level_passes += a_levels; h->stats.lk_iterations += a_iters; h->stats.lk_points += a_points; h->stats.tracked_features += a_tracked;
}

// undistortedPts (feature_tracker.cpp:797-808) for the listed sequences whose camera is no pinhole, in one launch behind the selection: every row of LK's points
// (tracked or not: the host picks by row) and the new corners, where they lie on the device.  d_npts is this call's only if LK ran, d_out_n only if the
// detection did; a table without counts is not lifted.
static_assert(sizeof(float2) == sizeof(gfcam::Pair) && alignof(float2) == alignof(gfcam::Pair), "float2 tables are passed as tables of gfcam::Pair");
static gfcam::Pair* pairs(float2* p) { return reinterpret_cast<gfcam::Pair*>(p); }
static int launch_lift(Call& c) {
    gf_tracker* h = c.h;
    gfcam::LiftArgs A{};
    A.cams = h->d_cams.p; A.cam_of = h->d_cam_of.p; A.first = nullptr; A.cap = h->cap; A.batch = c.N; A.n_sets = 2;
    A.set[0] = gfcam::LiftSet{pairs(h->d_cur_pts.p), c.any_prev ? h->d_npts.p : nullptr, pairs(h->d_un_lk.p), nullptr};
    A.set[1] = gfcam::LiftSet{pairs(h->d_out_pts.p), c.any_want ? h->d_out_n.p : nullptr, pairs(h->d_un_out.p), nullptr};
    // the right points of the call's stereo sequences, where the stereo kernel left them: one more list entry of the same launch, with the right cameras
    const gfcam::LiftSet right{pairs(h->d_st_pts.p), h->d_st_n.p, pairs(h->d_st_un.p), nullptr, h->d_st_cams.p, h->d_st_cam_of.p};
    if (!c.lift) { A.n_sets = 1; A.set[0] = right; }   // no left camera is lifted on the device: the right set alone, which brings its own cameras and list (A.cams / A.cam_of may be null tables then and are not read)
    else if (c.n_st_lift) { A.n_sets = 3; A.set[2] = right; }
    if (!c.n_st_lift && !c.any_prev && !c.any_want) return GF_OK;
    h->lift_launches++; h->lift_sequences += c.n_lift + c.n_st_lift;
    return camera_lift_launch(A, h->cap, h->stream);
}

// Shi-Tomasi top-up (feature_tracker.cpp:190-206) for the sequences that want corners.  Returns with the stream drained.
static int run_detect(Call& c) {
    gf_tracker* h = c.h;
    const int N = c.N, cap = h->cap;
    const bool prof = h->profiling;
    HandOver& ho = c.ho;
    if (c.any_want) {
        ho.down(h->d_det, h->h_det, N);
        c.add_refs();
        ho.down(h->d_centers, h->h_centers, (size_t)N * cap);
        ho.down(h->d_ncenters, h->h_ncenters, N);
        ho.down(h->d_want, h->h_want, N);
        if (h->d_seq_md.p) ho.down(h->d_seq_md, h->h_seq_md, N);
        ho.down(h->d_out_n, h->h_out_n, N);   // zeros (book_after_lk): a sequence that neither selection kernel serves reads 0, not an earlier call's count
        if (c.lift) ho.down(h->d_cam_of, h->h_cam_of, N);
        if (c.n_stereo) stereo_down(c);
        if (int rc = ho.flush()) return rc;
        HIPCHK(hipMemsetAsync(h->d_maxkey.p, 0, N * sizeof(unsigned), h->stream));
        HIPCHK(hipMemsetAsync(h->d_cand_count.p, 0, N * sizeof(int), h->stream));
        if (prof) HIPCHK(hipEventRecord(h->ev[4], h->stream));
        if (c.sized) launch_detect_sized(h, N, detect_args(h), h->size_plan.max_w, h->size_plan.max_h); else launch_detect(h, N, detect_args(h));
        // the sequences that want a handful of corners (every frame but the first ones): one maximum per corner instead of a sort (select_topk_kernel; GF_SELECT_TOPK=0: off)
        int max_want = 0;
        for (int i = 0; i < N; i++) max_want = std::max(max_want, h->h_want.p[i]);
        const bool topk = h->select_topk, sort = !topk || max_want > kTopKMax;
        const SelectArgs S = select_args(h, c.kdepth, topk ? 1 : 0);
        if (c.sized) launch_select_sized(h, N, S, topk, sort); else if (c.in.depth_by_refs()) launch_select<true>(h, N, S, topk, sort); else launch_select<false>(h, N, S, topk, sort);
        HIPCHK(hipGetLastError());
        if (c.n_stereo) if (int rc = launch_stereo(c)) return rc;
        if (c.n_sd) if (int rc = launch_stereo_depth(c)) return rc;
        if (c.lift || c.n_st_lift) if (int rc = launch_lift(c)) return rc;
        if (c.n_stereo) stereo_up(c);
        ho.up(h->h_out_n, h->d_out_n, N);
        ho.up(h->h_out_pts, h->d_out_pts, (size_t)N * cap);
        ho.up(h->h_out_depth, h->d_out_depth, (size_t)N * cap);
        ho.up(h->h_cand_count, h->d_cand_count, N);
        if (c.lift) { ho.up(h->h_un_lk, h->d_un_lk, (size_t)N * cap); ho.up(h->h_un_out, h->d_un_out, (size_t)N * cap); }
        if (int rc = ho.flush()) return rc;
    }
    if (prof && !c.any_want) HIPCHK(hipEventRecord(h->ev[4], h->stream));
    if ((c.lift || c.n_stereo) && !c.any_want) {   // no sequence wants corners: the tracked points alone (the counts of new corners go down as the zeros book_after_lk wrote)
        if (c.lift) ho.down(h->d_cam_of, h->h_cam_of, N);
        if (c.n_stereo) { stereo_down(c); ho.down(h->d_out_n, h->h_out_n, N); }
        if (int rc = ho.flush()) return rc;
        if (c.n_stereo) if (int rc = launch_stereo(c)) return rc;
        if (c.n_sd) if (int rc = launch_stereo_depth(c)) return rc;
        if (c.lift || c.n_st_lift) if (int rc = launch_lift(c)) return rc;
        if (c.lift) ho.up(h->h_un_lk, h->d_un_lk, (size_t)N * cap);
        if (c.n_stereo) stereo_up(c);
        if (int rc = ho.flush()) return rc;
    }
    if (prof) HIPCHK(hipEventRecord(h->ev[5], h->stream));
    c.lap(h->stats.ms_host_mid);
    HIPCHK(hipStreamSynchronize(h->stream));
    c.lap(h->stats.ms_wait_detect);
    return GF_OK;
}

static int read_profile(Call& c) {   // gf_tracker_set_profiling: the stages' times from the events of this call
    gf_tracker* h = c.h;
    float ms = 0;
    hipEvent_t from = h->ev[0];   // the stages ahead of the pyramid, each from where the one before it ended
    if (c.did_cvt) { HIPCHK(hipEventElapsedTime(&ms, from, h->ev[8])); h->stats.ms_convert += ms; from = h->ev[8]; }
    if (c.did_eq) { HIPCHK(hipEventElapsedTime(&ms, from, h->ev[7])); h->stats.ms_equalize += ms; from = h->ev[7]; }
    HIPCHK(hipEventElapsedTime(&ms, from, h->ev[1])); h->stats.ms_pyramid += ms;
    if (c.any_prev) { HIPCHK(hipEventElapsedTime(&ms, h->ev[2], h->ev[3])); h->stats.ms_lk += ms; }
    HIPCHK(hipEventElapsedTime(&ms, h->ev[4], h->ev[5])); h->stats.ms_detect += ms;
    HIPCHK(hipEventElapsedTime(&ms, h->ev[0], h->ev[5])); h->stats.ms_total_gpu += ms;
    return GF_OK;
}

// The candidate capacity, and which branch of the corner selection served each sequence (the kernels' own tests on the same numbers).
static int check_candidates(Call& c) {
    gf_tracker* h = c.h;
    for (int i = 0; i < c.N; i++) {
        if (h->h_want.p[i] > 0 && h->h_cand_count.p[i] > h->cand_cap)
            return set_err(GF_ERR_CAPACITY, "sequence %d: %d corner candidates exceed capacity %d", c.seq[i], h->h_cand_count.p[i], h->cand_cap);
        const int want = h->h_want.p[i], n = std::min(h->h_cand_count.p[i], h->cand_cap);
        if (want <= 0 || n <= 0) continue;
        if (h->select_topk && want <= kTopKMax) { if (n > 1024 * kTopKQ) h->stats.select_streamed++; }
        else {
            int npow2 = 64;
            while (npow2 < n) npow2 <<= 1;
            if (npow2 > h->sort_cap) h->stats.select_global_sort++;
        }
    }
    return GF_OK;
}

// Host bookkeeping behind the detection (after_detect, gf_track_host.hpp) per listed sequence on the pool: the sequences' new state and the caller's featureFrames.
static int book_after_detect(Call& c, gf_feature_obs* out, int cap_out, int* n_out) {
    gf_tracker* h = c.h;
    const int cap = h->cap;
    const bool have_depth = c.in.have_depth();
    std::atomic<int> a_overflow{-1};
    std::atomic<long long> a_out{0}, a_st_points{0}, a_st_matched{0};
    std::atomic<long long> a_sd[gfsd::kReasons];
    for (auto& a : a_sd) a = 0;
    h->pool->parallel_for(c.N, [&](int b) {   // b: list position
        const int q = c.seq[b];
        const DetectRows r{row(h->h_out_pts, b, cap), c.in.kernel_samples(h->h_out_depth, b, cap), h->h_want.p[b] > 0 ? h->h_out_n.p[b] : 0, c.in.host_image(b, h->par[q]), c.in.host_dstride};
        const bool own = !h->cam_on.empty() && h->cam_on[q], dev = own && c.lift && h->lifts_on_device(q);
        const bool stereo = c.n_stereo && h->h_st_right_of.p[b] >= 0;   // the frame came with a right image: the stage runs (after_detect, at the reference's place)
        const StereoRows sr{stereo ? row(h->h_st_pts, b, cap) : nullptr, stereo ? h->h_st_status.p + (size_t)b * cap : nullptr, stereo ? &h->st_cam[q] : nullptr,
                            stereo && h->h_st_cam_of.p[b] >= 0 ? row(h->h_st_un, b, cap) : nullptr};
        // the depth the matches determine (gf_tracker_set_seq_stereo_depth): the kernel's rows, or with GF_STEREO_DEPTH_HOST=1 the same function inside stereo_stage
        const bool sd_on = h->stereo_depth_on(q), sd_dev = sd_on && stereo && !h->sd_host;
        long long census[gfsd::kReasons] = {0};
        gfcam::Camera sd_left{}; gfsd::Rig sd_rig{};
        if (sd_on && stereo && h->sd_host) { sd_left = reject_f_camera(h, q); sd_rig = gfsd::rig_of(h->sd_cfg[q]); }
        const StereoDepthRows sdr{sd_dev ? h->h_sd_mm.p + (size_t)b * cap : nullptr, sd_dev ? h->h_sd_why.p + (size_t)b * cap : nullptr, &sd_left, &sd_rig,
                                  sd_on && h->sd_cfg[q].right_obs != 0, census};
        const Packed p = after_detect(h->seq[q], h->par[q], r, have_depth && !h->stereo_on(q), out + (size_t)b * cap_out, cap_out, own ? &h->cam[q] : nullptr,
                                      dev ? row(h->h_un_lk, b, cap) : nullptr, dev ? row(h->h_un_out, b, cap) : nullptr, stereo ? &sr : nullptr, sd_on ? &sdr : nullptr);
        if (stereo) { a_st_points += (long long)h->seq[q].prev_pts.size(); a_st_matched += (long long)h->seq[q].ids_right.size(); }
        if (sd_on && stereo) for (int k = 0; k < gfsd::kReasons; k++) a_sd[k] += census[k];
        if (h->seq[q].show_track) (void)record_track(h->seq[q], h->boxes.empty() ? nullptr : h->boxes[q].data(), h->boxes.empty() ? 0 : (int)h->boxes[q].size());   // a refused list: the sequence has no picture of this frame, and keeps the reason (draw_why)
        if (p.overflow >= 0) a_overflow = p.overflow;
        n_out[b] = p.written;
        a_out += p.written;
    });
    if (a_overflow.load() >= 0) return set_err(GF_ERR_CAPACITY, "output capacity %d < %d features", cap_out, a_overflow.load());
    h->stats.output_features += a_out;
    if (c.n_stereo) { h->st_stats.calls++; h->st_stats.points += a_st_points; h->st_stats.matched += a_st_matched; }
    if (c.n_sd) {
        gf_stereo_depth_stats& s = h->sd_stats;
        s.calls++;
        for (int k = 0; k < gfsd::kReasons; k++) s.points += a_sd[k];
        s.with_depth += a_sd[gfsd::kOk]; s.no_match += a_sd[gfsd::kNoMatch]; s.lift += a_sd[gfsd::kLift]; s.parallax += a_sd[gfsd::kParallax];
        s.behind += a_sd[gfsd::kBehind]; s.epipolar += a_sd[gfsd::kEpipolar]; s.range += a_sd[gfsd::kRange];
    }
    return GF_OK;
}

// One frame for each of the `count` listed sequences (seq: checked by check_list); sequences that are not listed keep their whole state.  Everything the caller hands
// in or gets back (t, the frames of `in`, out, n_out) and every hand-over table of the handle is indexed by the position i in the list, so the work and the bytes of
// a call follow `count`; only h->seq[], h->par[] and the pyramid pairs are indexed by the sequence seq[i].
static int track_core(gf_tracker* h, int count, const int* seq, const double* t, const FrameInput& in, gf_feature_obs* out, int cap_out, int* n_out) {
    if (count == 0) return GF_OK;
    Call c{h, count, seq, in, HandOver(h->copy_lists, h->stream)};
    if (h->fmt_any) { plan_call(h, count, seq); c.mixed = !h->plan.homogeneous; }
    if (h->size_any) { plan_sizes(h, count, seq); c.sized = h->size_plan.sized; if (c.sized) c.mixed = false; }   // the sized front walks the formats itself
    for (int i = 0; i < count; i++) h->h_cur.p[i] = 2 * seq[i] + begin_frame(h->seq[seq[i]], t[i]);   // the new frame goes to the sequence's other pyramid
    if (int rc = publish(c)) return rc;
    if (int rc = launch_front(c)) return rc;
    if (c.n_reg) if (int rc = launch_depth_reg(c)) return rc;
    if (c.n_stereo) if (int rc = launch_right_pyramids(c)) return rc;
    if (int rc = run_lk(c)) return rc;
    if (int rc = redo_fallback(c)) return rc;
    book_after_lk(c);
    if (int rc = run_detect(c)) return rc;
    h->box_pending = false;   // the stream is drained: a box setter's staging has been read
    if (c.n_reg) { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, h->ev_dreg[0], h->ev_dreg[1])); h->dreg_ms += ms; }
    for (int k = 0; k < c.rf_launches; k++) { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, h->ev_rf[2 * k], h->ev_rf[2 * k + 1])); h->rf_stats.kernel_ms += ms; }
    if (h->profiling) if (int rc = read_profile(c)) return rc;
    if (c.any_want) if (int rc = check_candidates(c)) return rc;
    if (int rc = book_after_detect(c, out, cap_out, n_out)) return rc;
    h->stats.frames++;
    h->stats.sequence_frames += count;
    c.lap(h->stats.ms_host_post);
    return GF_OK;
}

}  // namespace gf

// =============================================================================== C-ABI
extern "C" {

const char* gf_last_error(void) { return gf::g_err.c_str(); }

int gf_device_count(int* n) {
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *n = 0; return gf::set_err(GF_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *n = c;
    return GF_OK;
}
int gf_set_device(int device) { HIPCHK(hipSetDevice(device)); return GF_OK; }

int gf_tracker_create(const gf_tracker_cfg* cfg, gf_tracker** out) {
    if (!cfg || !out) return gf::set_err(GF_ERR_INVALID, "null argument");
    *out = nullptr;
    if (cfg->width < 32 || cfg->height < 32 || cfg->width % 4 || cfg->batch < 1 || cfg->max_cnt < 1 || cfg->min_dist < 0 || cfg->min_dist > gf::kMaxRadius)
        return gf::set_err(GF_ERR_INVALID, "unsupported tracker configuration (width %% 4 == 0, width/height >= 32, 0 <= min_dist <= %d)", gf::kMaxRadius);
    if (cfg->equalize != 0 && cfg->equalize != 1) return gf::set_err(GF_ERR_INVALID, "gf_tracker_cfg.equalize must be 0 or 1, got %d", cfg->equalize);
    if (!gfpix::valid(cfg->pixel_format)) return gf::set_err(GF_ERR_INVALID, "gf_tracker_cfg.pixel_format must be one of GF_PIX_MONO8 (0) .. GF_PIX_BGRA8 (4) or GF_PIX_BAYER_RGGB8 (8) .. GF_PIX_MONO16 (14), got %d", cfg->pixel_format);
    if (int rc = gf::require_device()) return rc;
    std::unique_ptr<gf_tracker> h(new gf_tracker());
    h->cfg = *cfg;
    h->ch = gfpix::channels(cfg->pixel_format);
    h->B = cfg->batch;
    h->cap = (cfg->max_cnt + 3) & ~3;
    gf::build_geom(cfg->width, cfg->height, h->G);
    gf::make_disk_table(cfg->min_dist, h->disk);
    h->seq.resize(h->B);
    h->par.assign(h->B, gfseq::of_handle(*cfg));
    h->fmt.assign(h->B, gfseqfmt::of_handle(*cfg));
    h->raw_ch = h->ch;
    h->sizes.init(cfg->width, cfg->height, h->B);
    h->ident.resize(h->B);
    for (int b = 0; b < h->B; b++) h->ident[b] = b;
    {
        // default: up to 16 threads out of this rank's share of the node (a frame of 256 sequences spends 1.3 ms in the bookkeeping with 4 threads, 0.5 ms with 16)
        const auto [hw, share] = gf::rank_host_share();   // ... of the hardware threads this process can really use (its affinity mask and its container's CPU quota, not the box)
        int nthr = std::max(1, std::min(16, hw / (2 * share)));
        if (const char* e = getenv("GF_HOST_THREADS")) nthr = atoi(e);
        nthr = std::max(1, std::min(nthr, std::max(hw, 1)));
        int dev = 0;
        (void)hipGetDevice(&dev);
        h->pool.reset(new gf::HostPool(h->B >= 8 ? nthr - 1 : 0, dev));
        h->copy_lists = !(getenv("GF_TRACKER_COPIES") && atoi(getenv("GF_TRACKER_COPIES")) != 0);
        h->pyr_head = !(getenv("GF_PYR_HEAD") && atoi(getenv("GF_PYR_HEAD")) == 0);
        h->select_topk = !(getenv("GF_SELECT_TOPK") && atoi(getenv("GF_SELECT_TOPK")) == 0);
        if (const char* e = getenv("GF_CAMERA_LIFT_HOST")) h->lift_mode = atoi(e) != 0 ? 1 : 0;
        if (const char* e = getenv("GF_REJECT_F_HOST")) h->rf_host = atoi(e) != 0;
        if (const char* e = getenv("GF_STEREO_DEPTH_HOST")) h->sd_host = atoi(e) != 0;
        if (const char* e = getenv("GF_LK_POINTS")) { const int v = atoi(e); if (v == 1 || v == 2 || v == 4) h->lk_points = v; }
    }
    const int W = cfg->width, H = cfg->height, B = h->B, cap = h->cap;
    int cc = 1024;
    while (cc < (W * H) / 2) cc <<= 1;
    h->cand_cap = cc;
    h->eig_stride = ((size_t)W * H + 3) & ~(size_t)3;
    h->mask_stride = ((size_t)W * H + 15) & ~(size_t)15;
    const int cell = std::max(cfg->min_dist, 1);
    const int gw = (W + cell - 1) / cell, gh = (H + cell - 1) / cell;
    const size_t grid_lds = (size_t)((gw * gh + 3) & ~3) * 2 + (size_t)cap * 3 * 2 + 64;
    h->sort_cap = gf::kSortLds;
    while (h->sort_cap > 64 && (size_t)h->sort_cap * 8 + grid_lds > 160 * 1024) h->sort_cap >>= 1;
    h->select_lds = (size_t)h->sort_cap * 8 + grid_lds;
    if (h->select_lds > 160 * 1024) return gf::set_err(GF_ERR_INVALID, "min_dist %d too small for the selection grid at %dx%d", cfg->min_dist, W, H);
    HIPCHK(hipStreamCreateWithFlags(&h->stream.s, hipStreamNonBlocking));
    for (auto& e : h->ev) HIPCHK(hipEventCreate(&e.e));
    // The allocations as explicit statements, in this order: a buffer's place in the sequence decides which memory it gets.
    HIPCHK(h->d_img.alloc((size_t)B * 2 * h->G.img_bytes));
    HIPCHK(h->d_raw.alloc((size_t)B * W * H * h->ch));
    if (cfg->pixel_format) HIPCHK(h->d_cvt.alloc((size_t)B * W * H));
    if (cfg->equalize) { HIPCHK(h->d_eq.alloc((size_t)B * W * H)); HIPCHK(h->d_eq_lut.alloc(gf::clahe_lut_bytes(B, gf::kClaheTiles, gf::kClaheTiles))); }
    // (no device copy of the depth images: the host entry points sample them on the host, the device entry point reads the caller's device pointer)
    HIPCHK(h->d_mask.alloc(h->mask_stride));  // explicit masks exist only in the gf_good_features building block
    HIPCHK(h->d_eig.alloc(h->eig_stride));    // response image materialised only by gf_min_eigen_val
    HIPCHK(h->d_cand.alloc((size_t)B * h->cand_cap));
    HIPCHK(h->d_status.alloc((size_t)B * cap)); HIPCHK(h->d_fwd_status.alloc((size_t)B * cap)); HIPCHK(h->d_seqmask.alloc(2 * (size_t)B));
    HIPCHK(h->d_npts.alloc(B)); HIPCHK(h->d_cand_count.alloc(B)); HIPCHK(h->d_want.alloc(B)); HIPCHK(h->d_ncenters.alloc(B)); HIPCHK(h->d_out_n.alloc(B));
    HIPCHK(h->d_depth_out.alloc((size_t)B * cap)); HIPCHK(h->d_out_depth.alloc((size_t)B * cap));
    HIPCHK(h->d_prev_pts.alloc((size_t)B * cap)); HIPCHK(h->d_init_pts.alloc((size_t)B * cap)); HIPCHK(h->d_cur_pts.alloc((size_t)B * cap)); HIPCHK(h->d_out_pts.alloc((size_t)B * cap));
    HIPCHK(h->d_counters.alloc((size_t)B * cap * 2)); HIPCHK(h->d_maxkey.alloc(B)); HIPCHK(h->d_centers.alloc((size_t)B * cap));
    HIPCHK(h->h_npts.alloc(B)); HIPCHK(h->h_want.alloc(B)); HIPCHK(h->h_ncenters.alloc(B)); HIPCHK(h->h_out_n.alloc(B)); HIPCHK(h->h_cand_count.alloc(B));
    HIPCHK(h->h_prev_pts.alloc((size_t)B * cap)); HIPCHK(h->h_init_pts.alloc((size_t)B * cap)); HIPCHK(h->h_cur_pts.alloc((size_t)B * cap)); HIPCHK(h->h_out_pts.alloc((size_t)B * cap));
    HIPCHK(h->h_status.alloc((size_t)B * cap)); HIPCHK(h->h_fwd_status.alloc((size_t)B * cap)); HIPCHK(h->h_seqmask.alloc(2 * (size_t)B)); HIPCHK(h->h_depth_out.alloc((size_t)B * cap)); HIPCHK(h->h_out_depth.alloc((size_t)B * cap));
    HIPCHK(h->h_counters.alloc((size_t)B * cap * 2)); HIPCHK(h->h_centers.alloc((size_t)B * cap));
    HIPCHK(h->d_cur.alloc(B)); HIPCHK(h->h_cur.alloc(B)); HIPCHK(h->d_det.alloc(B)); HIPCHK(h->h_det.alloc(B));   // behind the others, whose places relative to each other stay as measured
    HIPCHK(hipMemsetAsync(h->d_img.p, 0, h->d_img.n, h->stream));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(gf::select_corners_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->select_lds));
    HIPCHK(hipStreamSynchronize(h->stream));
    *out = h.release();
    return GF_OK;
}

int gf_tracker_destroy(gf_tracker* h) { delete h; return GF_OK; }

// ---- trackImage (feature_tracker.h:47) for the listed sequences of a handle.  t[i], gray[i], depth[i], out[i * cap ..], n_out[i] belong to sequence seq[i].
int gf_tracker_track_some_device(gf_tracker* h, int count, const int* seq, const double* t, const void* d_gray, const void* d_depth, gf_feature_obs* out, int cap,
                                 int* n_out) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (int rc = gf::check_list(h, count, seq)) return rc;
    if (count == 0) return GF_OK;
    if (!t || !d_gray || !out || !n_out) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (int rc = gf::refuse_registered(h, "gf_tracker_track_some_device", count, seq, d_depth != nullptr)) return rc;
    return gf::track_core(h, count, seq, t, gf::FrameInput::device((const uint8_t*)d_gray, (const uint16_t*)d_depth), out, cap, n_out);
}

// ---- the same with one gf_frame_ref per listed sequence (gf_frame_ref.hpp)
namespace gf {
static int refs_ready(gf_tracker* h) {   // the first _refs call of a handle: the table and its device copy, and the _refs form of the sort kernel gets the LDS the handle's own got
    if (h->h_refs.p) return GF_OK;
    DevBuf<gf_frame_ref> dev; PinBuf<gf_frame_ref> pin;
    HIPCHK(dev.alloc((size_t)2 * h->B)); HIPCHK(pin.alloc((size_t)2 * h->B));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(select_corners_refs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->select_lds));
    h->d_refs = std::move(dev); h->h_refs = std::move(pin);
    return GF_OK;
}
// every entry of a table of `count`, or GF_ERR_INVALID naming the list position; what: "gray", "depth" or "mask"
// own_size: bytes per pixel of an image that has the sequence's own frame size where a setter gave it one (0: row_bytes holds whatever the sizes)
static int check_refs(const gf_tracker* h, int count, const int* seq, const gf_frame_ref* refs, size_t row_bytes, bool u16, const char* what, size_t own_size = 0) {
    const bool own_rows = row_bytes == 0;   // gray frames: a row of each sequence's own format (gf_tracker_set_seq_format)
    for (int i = 0; i < count; i++) {
        if (own_rows) row_bytes = gfseqfmt::row_bytes(h->cfg.width, h->fmt[seq[i]].pixel_format);
        if (h->size_any && own_size) row_bytes = own_rows ? gfseqfmt::row_bytes(seq_width(h, seq[i]), h->fmt[seq[i]].pixel_format) : (size_t)seq_width(h, seq[i]) * own_size;   // a row of the sequence's own width (gf_tracker_set_seq_size)
        const bool raw_depth = u16 && !h->dreg_on.empty() && h->dreg_on[seq[i]];   // the raw frame of the sequence's depth camera (gf_tracker_set_seq_depth_reg)
        const size_t need = raw_depth ? (size_t)h->dreg[seq[i]].width * 2 : row_bytes;
        if (u16 && h->stereo_on(seq[i])) {   // the second entry of a stereo sequence is its right frame: 8-bit, any pointer or pitch, or null (`_img1.empty()`)
            const size_t rrow = (size_t)seq_width(h, seq[i]);
            const gfref::Verdict rv = gfref::check(refs[i], rrow, false, true);
            if (rv != gfref::kOk)
                return set_err(GF_ERR_INVALID, "right frame at list position %d (sequence %d): %s (data %p, pitch %zu bytes, a row is %zu bytes)", i, seq[i], gfref::verdict_text(rv), refs[i].data, refs[i].pitch, rrow);
            continue;
        }
        const gfref::Verdict v = gfref::check(refs[i], need, u16, u16 && !h->par[seq[i]].depth_cam);
        if (v != gfref::kOk)
            return set_err(GF_ERR_INVALID, "%s frame at list position %d (sequence %d): %s (data %p, pitch %zu bytes, a row is %zu bytes)", raw_depth ? "raw depth" : what, i, seq[i], gfref::verdict_text(v), refs[i].data, refs[i].pitch, need);
    }
    return GF_OK;
}
}  // namespace gf

int gf_tracker_track_some_device_refs(gf_tracker* h, int count, const int* seq, const double* t, const gf_frame_ref* gray, const gf_frame_ref* depth,
                                      gf_feature_obs* out, int cap, int* n_out) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (int rc = gf::check_list(h, count, seq)) return rc;
    if (count == 0) return GF_OK;
    if (!gray) return gf::set_err(GF_ERR_INVALID, "null table of gray frames");
    if (!t || !out || !n_out) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (int rc = gf::check_refs(h, count, seq, gray, 0, false, "gray", 1)) return rc;
    if (depth) if (int rc = gf::check_refs(h, count, seq, depth, (size_t)h->cfg.width * 2, true, "depth", 2)) return rc;
    if (int rc = gf::refs_ready(h)) return rc;
    return gf::track_core(h, count, seq, t, gf::FrameInput::by_refs(gray, depth), out, cap, n_out);
}

int gf_tracker_track_batch_device_refs(gf_tracker* h, const double* t, const gf_frame_ref* gray, const gf_frame_ref* depth, gf_feature_obs* out, int cap, int* n_out) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    return gf_tracker_track_some_device_refs(h, h->B, h->ident.data(), t, gray, depth, out, cap, n_out);
}

int gf_tracker_track_some(gf_tracker* h, int count, const int* seq, const double* t, const uint8_t* const* gray, int stride, const uint16_t* const* depth, int dstride,
                          gf_feature_obs* out, int cap, int* n_out) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (int rc = gf::check_list(h, count, seq)) return rc;
    if (count == 0) return GF_OK;
    if (!t || !gray || !out || !n_out) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (int rc = gf::refuse_registered(h, "gf_tracker_track_some", count, seq, depth != nullptr)) return rc;
    bool have_depth = false, sized = false;
    if (int rc = gf::check_host_frames(h, count, seq, gray, stride, depth, dstride, &have_depth, &sized)) return rc;   // refuse before the first copy
    const size_t row = (size_t)h->cfg.width * h->ch;   // bytes of a row of the handle's pixel format
    const int H = h->cfg.height;
    if (sized) { if (int rc = gf::copy_host_frames_sized(h, count, seq, gray, stride, h->d_raw.p, h->stream)) return rc; }
    else if (h->fmt_any) { if (int rc = gf::copy_host_frames(h, count, seq, gray, stride, h->d_raw.p, h->stream)) return rc; }
    else for (int i = 0; i < count; i++) HIPCHK(hipMemcpy2DAsync(h->d_raw.p + (size_t)i * row * H, row, gray[i], stride, row, H, hipMemcpyHostToDevice, h->stream));
    // the depth image stays where it is: its <= max_cnt samples are taken on the host (after_lk, after_detect)
    return gf::track_core(h, count, seq, t, gf::FrameInput::with_host_depth(h->d_raw.p, have_depth ? depth : nullptr, dstride), out, cap, n_out);
}

// The host-image boundary (trackImage(const cv::Mat&), feature_tracker.h:47) without serialising on the bus: the images of frame k + 1 go to the second pair of
// frame buffers on a copy stream while frame k's kernels run; gf_tracker_track_prefetched then only waits for that copy.  The host images must stay valid until
// the matching gf_tracker_track_prefetched returns, and only page-locked memory (gf_host_alloc / hipHostRegister) makes the copy asynchronous.  The staged frame
// remembers its list: gf_tracker_track_prefetched advances exactly the sequences whose images were staged.
int gf_tracker_prefetch_some(gf_tracker* h, int count, const int* seq, const uint8_t* const* gray, int stride, const uint16_t* const* depth, int dstride) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (int rc = gf::check_list(h, count, seq)) return rc;
    if (count > 0 && !gray) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (int rc = gf::refuse_registered(h, "gf_tracker_prefetch_some", count, seq, depth != nullptr)) return rc;
    bool have_depth = false, sized = false;
    if (int rc = gf::check_host_frames(h, count, seq, gray, stride, depth, dstride, &have_depth, &sized)) return rc;
    const size_t row = (size_t)h->cfg.width * h->ch;   // bytes of a row of the handle's pixel format
    const int H = h->cfg.height;
    if (h->pf_count >= 2) return gf::set_err(GF_ERR_CAPACITY, "two frames are staged already: gf_tracker_track_prefetched has to consume one first");
    if (!h->copy_stream) {
        HIPCHK(hipStreamCreateWithFlags(&h->copy_stream.s, hipStreamNonBlocking));
        for (auto& e : h->ev_copy) HIPCHK(hipEventCreateWithFlags(&e.e, hipEventDisableTiming));
        HIPCHK(h->d_raw2.alloc((size_t)h->B * h->cfg.width * H * h->raw_ch));   // the pair of d_raw: room for the widest format in force
    }
    const int slot = (h->pf_head + h->pf_count) & 1;      // a pair no frame in flight uses: track calls return when their frame is done
    uint8_t* raw = slot ? h->d_raw2.p : h->d_raw.p;
    // images that sit back to back in one allocation (a pinned ring of frames) go as ONE copy per plane: 256 separate 2-D copies cost more host time than the bus needs
    bool contig = (size_t)stride == row && !h->fmt_any && !sized;
    for (int i = 1; i < count && contig; i++) contig = gray[i] == gray[0] + (size_t)i * row * H;
    if (sized) { if (int rc = gf::copy_host_frames_sized(h, count, seq, gray, stride, raw, h->copy_stream)) return rc; }
    else if (h->fmt_any) { if (int rc = gf::copy_host_frames(h, count, seq, gray, stride, raw, h->copy_stream)) return rc; }
    else if (contig && count > 0) HIPCHK(hipMemcpyAsync(raw, gray[0], (size_t)count * row * H, hipMemcpyHostToDevice, h->copy_stream));
    else for (int i = 0; i < count; i++) HIPCHK(hipMemcpy2DAsync(raw + (size_t)i * row * H, row, gray[i], stride, row, H, hipMemcpyHostToDevice, h->copy_stream));
    HIPCHK(hipEventRecord(h->ev_copy[slot], h->copy_stream));
    // the depth images do not travel: gf_tracker_track_prefetched samples them on the host (they must stay valid until it returns, like the gray images until the copy is done)
    h->pf_depth[slot] = have_depth; if (have_depth) h->pf_hdepth[slot].assign(depth, depth + count); else h->pf_hdepth[slot].clear();
    h->pf_hdstride[slot] = dstride;
    h->pf_seq[slot].assign(seq, seq + count);   // an empty list is staged too: the caller's prefetch / track_prefetched pairs stay in step
    h->pf_count++;
    return GF_OK;
}

int gf_tracker_track_prefetched(gf_tracker* h, const double* t, gf_feature_obs* out, int cap, int* n_out) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (!h->pf_count) return gf::set_err(GF_ERR_INVALID, "gf_tracker_track_prefetched without a staged frame (call gf_tracker_prefetch_batch or _prefetch_some first)");
    const int slot = h->pf_head;
    const std::vector<int>& seq = h->pf_seq[slot];
    if (!seq.empty() && (!t || !out || !n_out)) return gf::set_err(GF_ERR_INVALID, "null argument");
    HIPCHK(hipStreamWaitEvent(h->stream, h->ev_copy[slot], 0));
    h->pf_head ^= 1; h->pf_count--;
    return gf::track_core(h, (int)seq.size(), seq.data(), t, gf::FrameInput::with_host_depth(slot ? h->d_raw2.p : h->d_raw.p, h->pf_depth[slot] ? h->pf_hdepth[slot].data() : nullptr, h->pf_hdstride[slot]), out, cap, n_out);
}

// ---- the lock-step forms: the same calls with every sequence listed in order
int gf_tracker_track_batch_device(gf_tracker* h, const double* t, const void* d_gray, const void* d_depth, gf_feature_obs* out, int cap,
                                  int* n_out) {
    if (!h || !t || !d_gray || !out || !n_out) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (int rc = gf::refuse_registered(h, "gf_tracker_track_batch_device", h->B, h->ident.data(), d_depth != nullptr)) return rc;
    return gf_tracker_track_some_device(h, h->B, h->ident.data(), t, d_gray, d_depth, out, cap, n_out);
}

int gf_tracker_track_batch(gf_tracker* h, const double* t, const uint8_t* const* gray, int stride, const uint16_t* const* depth, int dstride,
                           gf_feature_obs* out, int cap, int* n_out) {
    if (!h || !t || !gray || !out || !n_out) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (int rc = gf::refuse_registered(h, "gf_tracker_track_batch", h->B, h->ident.data(), depth != nullptr)) return rc;
    return gf_tracker_track_some(h, h->B, h->ident.data(), t, gray, stride, depth, dstride, out, cap, n_out);
}

int gf_tracker_prefetch_batch(gf_tracker* h, const uint8_t* const* gray, int stride, const uint16_t* const* depth, int dstride) {
    if (!h || !gray) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (int rc = gf::refuse_registered(h, "gf_tracker_prefetch_batch", h->B, h->ident.data(), depth != nullptr)) return rc;
    return gf_tracker_prefetch_some(h, h->B, h->ident.data(), gray, stride, depth, dstride);
}

// page-locked host memory for frames that are handed to gf_tracker_prefetch_batch / gf_tracker_track_batch (pageable memory makes hipMemcpyAsync synchronous)
int gf_host_alloc(size_t bytes, void** out) {
    if (!out || !bytes) return gf::set_err(GF_ERR_INVALID, "bad argument");
    if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) return gf::set_err(GF_ERR_HIP, "hipHostMalloc(%zu) failed", bytes);
    return GF_OK;
}
int gf_host_free(void* p) { gf::pinned_free(p); return GF_OK; }

// the list of one: any sequence of any handle
int gf_tracker_track(gf_tracker* h, int seq, double t, const uint8_t* gray, int stride, const uint16_t* depth, int dstride, gf_feature_obs* out,
                     int cap, int* n_out) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    const uint8_t* g[1] = {gray};
    const uint16_t* d[1] = {depth};
    if (seq >= 0 && seq < h->B) if (int rc = gf::refuse_registered(h, "gf_tracker_track", 1, &seq, depth != nullptr)) return rc;
    return gf_tracker_track_some(h, 1, &seq, &t, g, stride, depth ? d : nullptr, dstride, out, cap, n_out);
}

int gf_tracker_set_prediction(gf_tracker* h, int seq, const int* ids, const double* xyz, int n) {
    if (!h || seq < 0 || seq >= h->B || (n > 0 && (!ids || !xyz))) return gf::set_err(GF_ERR_INVALID, "bad argument");
    gf::set_prediction(h->seq[seq], h->par[seq], ids, xyz, n, !h->cam_on.empty() && h->cam_on[seq] ? &h->cam[seq] : nullptr);
    return GF_OK;
}

int gf_tracker_set_roi(gf_tracker* h, int seq, const uint8_t* mask, int stride) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    const int W = gf::seq_width(h, seq), H = gf::seq_height(h, seq);   // the mask is an image of the sequence's own size
    if (mask && stride < W) return gf::set_err(GF_ERR_INVALID, "a mask stride of %d bytes is shorter than a row of %d pixels", stride, W);
    if (!mask && !h->d_roi.p) return GF_OK;   // nothing to clear: the handle stays one that never had a region
    if (int rc = gf::roi_ready(h)) return rc;
    if (mask) {
        uint32_t* t = h->roi_bits.data() + (size_t)seq * h->roi_words;
        if (gf::seq_has_size(h, seq)) std::fill_n(t, h->roi_words, ~0u);   // the words its own geometry does not reach
        for (int band = 0; band < gfroi::bands(H); band++)
            for (int x = 0; x < W; x++)
                gfroi::pack_thread(mask, (size_t)stride, W, H, band, x, t);
        h->roi_has[seq] = 1;
    } else gf::roi_clear_host(h, seq);
    return gf::roi_upload(h, seq);
}

int gf_tracker_set_roi_some_device(gf_tracker* h, int count, const int* seq, const void* d_masks) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (int rc = gf::check_list(h, count, seq)) return rc;
    if (count == 0 || (!d_masks && !h->d_roi.p)) return GF_OK;
    if (int rc = gf::roi_ready(h)) return rc;
    if (!d_masks) {
        for (int i = 0; i < count; i++) { gf::roi_clear_host(h, seq[i]); if (int rc = gf::roi_upload(h, seq[i])) return rc; }
        return GF_OK;
    }
    const int W = h->cfg.width, H = h->cfg.height;
    if (gf::any_has_size(h, count, seq)) {   // masks of the sequences' own sizes, back to back: mask i at the sum of the masks before it
        gfsize::plan_list(h->size_plan, h->sizes, count, seq);
        for (int i = 0; i < count; i++) h->h_refs.p[i] = gf_frame_ref{static_cast<const uint8_t*>(d_masks) + h->size_plan.mask_off[i], (size_t)h->size_plan.w[i]};
        return gf::roi_pack_sized(h, count, seq);
    }
    HIPCHK(hipMemcpyAsync(h->d_roi_seq.p, seq, (size_t)count * sizeof(int), hipMemcpyHostToDevice, h->stream));
    gf::roi_pack_kernel<<<dim3((W + 255) / 256, gfroi::bands(H), count), 256, 0, h->stream>>>((const uint8_t*)d_masks, h->d_roi_seq.p, W, H, gf::roi_base_table(h), h->roi_words);
    HIPCHK(hipGetLastError());
    return gf::roi_packed(h, count, seq);
}

int gf_tracker_set_roi_some_device_refs(gf_tracker* h, int count, const int* seq, const gf_frame_ref* masks) {
    if (!masks) return gf_tracker_set_roi_some_device(h, count, seq, nullptr);   // clears, as there
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (int rc = gf::check_list(h, count, seq)) return rc;
    if (count == 0) return GF_OK;
    const int W = h->cfg.width, H = h->cfg.height;
    if (int rc = gf::check_refs(h, count, seq, masks, (size_t)W, false, "mask", 1)) return rc;
    if (int rc = gf::roi_ready(h)) return rc;
    if (int rc = gf::refs_ready(h)) return rc;
    for (int i = 0; i < count; i++) h->h_refs.p[i] = masks[i];
    if (gf::any_has_size(h, count, seq)) { gfsize::plan_list(h->size_plan, h->sizes, count, seq); return gf::roi_pack_sized(h, count, seq); }
    HIPCHK(hipMemcpyAsync(h->d_refs.p, h->h_refs.p, (size_t)count * sizeof(gf_frame_ref), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_roi_seq.p, seq, (size_t)count * sizeof(int), hipMemcpyHostToDevice, h->stream));
    gf::roi_pack_refs_kernel<<<dim3((W + 255) / 256, gfroi::bands(H), count), 256, 0, h->stream>>>(h->d_refs.p, h->d_roi_seq.p, W, H, gf::roi_base_table(h), h->roi_words);
    HIPCHK(hipGetLastError());
    return gf::roi_packed(h, count, seq);
}

int gf_tracker_get_roi(gf_tracker* h, int seq, uint8_t* mask, int stride, int* has) {
    if (!h || !has) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    const int W = gf::seq_width(h, seq), H = gf::seq_height(h, seq);   // a mask of the sequence's own size
    if (mask && stride < W) return gf::set_err(GF_ERR_INVALID, "a mask stride of %d bytes is shorter than a row of %d pixels", stride, W);
    const bool base = !h->roi_has.empty() && h->roi_has[seq];
    const int nb = h->boxes.empty() ? 0 : (int)h->boxes[seq].size();
    *has = base || nb > 0 ? 1 : 0;
    if (!*has || !mask) return GF_OK;
    const uint32_t* t = base ? h->roi_bits.data() + (size_t)seq * h->roi_words : nullptr;
    const gf_box* bx = nb ? h->boxes[seq].data() : nullptr;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) mask[(size_t)y * stride + x] = gfroi::allowed(t, bx, nb, W, x, y) ? 255 : 0;
    return GF_OK;
}

// ---- exclusion boxes (gf_roi.hpp): trackImagebox's boxes (feature_tracker.cpp:374, :565-599) as part of the region in force
int gf_tracker_set_boxes_some(gf_tracker* h, int count, const int* seq, const int* first, const gf_box* boxes) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (int rc = gf::check_box_lists(h, count, seq, first, boxes)) return rc;
    if (count == 0) return GF_OK;
    if (!h->d_roi_base.p && (!first || first[count] == 0)) return GF_OK;   // nothing to clear: the handle stays one that never had boxes
    if (int rc = gf::boxes_ready(h)) return rc;
    for (int i = 0; i < count; i++) {
        if (first) h->boxes[seq[i]].assign(boxes + first[i], boxes + first[i + 1]);
        else h->boxes[seq[i]].clear();
    }
    return gf::boxes_compose(h, count, seq);
}

int gf_tracker_get_boxes(gf_tracker* h, int seq, gf_box* boxes, int cap, int* n) {
    if (!h || !n) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    if (cap < 0 || (cap > 0 && !boxes)) return gf::set_err(GF_ERR_INVALID, "room for %d boxes at a null pointer", cap);
    *n = h->boxes.empty() ? 0 : (int)h->boxes[seq].size();
    for (int i = 0; i < *n && i < cap; i++) boxes[i] = h->boxes[seq][i];
    return GF_OK;
}

int gf_roi_boxes_batch(int batch, int width, int height, const int* first, const gf_box* boxes, const uint8_t* base_masks, uint8_t* out_masks) {
    if (batch < 1 || batch > 65535 || width < 1 || height < 1 || !first || !out_masks) return gf::set_err(GF_ERR_INVALID, "bad argument");
    if (first[0] != 0) return gf::set_err(GF_ERR_INVALID, "first[0] is %d, not 0", first[0]);
    for (int b = 0; b < batch; b++) {
        if (first[b + 1] < first[b]) return gf::set_err(GF_ERR_INVALID, "frame %d: first decreases from %d to %d", b, first[b], first[b + 1]);
        if (first[b + 1] - first[b] > GF_MAX_BOXES_PER_SEQ) return gf::set_err(GF_ERR_INVALID, "frame %d: %d boxes > GF_MAX_BOXES_PER_SEQ = %d", b, first[b + 1] - first[b], GF_MAX_BOXES_PER_SEQ);
    }
    const int total = first[batch];
    if (total > 0 && !boxes) return gf::set_err(GF_ERR_INVALID, "%d boxes listed but `boxes` is null", total);
    if (int rc = gf::require_device()) return rc;
    const size_t words = gfroi::words(width, height), px = (size_t)width * height;
    gf::DevBuf<uint32_t> d_base, d_out; gf::DevBuf<uint8_t> d_masks, d_stage; gf::DevBuf<int> d_ident;
    HIPCHK(d_out.fit((size_t)batch * words));
    std::vector<gf::RoiBoxJob> jobs(batch);
    for (int b = 0; b < batch; b++) jobs[b] = gf::RoiBoxJob{b, first[b], first[b + 1] - first[b], 0};
    const size_t job_bytes = (size_t)batch * sizeof(gf::RoiBoxJob);
    HIPCHK(d_stage.fit(job_bytes + (size_t)std::max(total, 1) * sizeof(gf_box)));
    HIPCHK(hipMemcpy(d_stage.p, jobs.data(), job_bytes, hipMemcpyHostToDevice));
    if (total > 0) HIPCHK(hipMemcpy(d_stage.p + job_bytes, boxes, (size_t)total * sizeof(gf_box), hipMemcpyHostToDevice));
    if (base_masks) {   // the base words by the tracker's packing kernel
        std::vector<int> ident(batch);
        for (int b = 0; b < batch; b++) ident[b] = b;
        HIPCHK(d_base.fit((size_t)batch * words)); HIPCHK(d_masks.fit((size_t)batch * px)); HIPCHK(d_ident.fit(batch));
        HIPCHK(hipMemcpy(d_masks.p, base_masks, (size_t)batch * px, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_ident.p, ident.data(), (size_t)batch * sizeof(int), hipMemcpyHostToDevice));
        gf::roi_pack_kernel<<<dim3((width + 255) / 256, gfroi::bands(height), batch), 256>>>(d_masks.p, d_ident.p, width, height, d_base.p, words);
        HIPCHK(hipGetLastError());
    }
    const gf::RoiBoxJob* d_jobs = reinterpret_cast<const gf::RoiBoxJob*>(d_stage.p);
    gf::roi_boxes_kernel<<<dim3((width + gf::kRoiBoxSpan - 1) / gf::kRoiBoxSpan, gfroi::bands(height), batch), gf::kRoiBoxPiece>>>(
        d_jobs, reinterpret_cast<const gf_box*>(d_jobs + batch), width, height, d_base.p, d_out.p, words);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    std::vector<uint32_t> table((size_t)batch * words);
    HIPCHK(hipMemcpy(table.data(), d_out.p, table.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int b = 0; b < batch; b++)
        for (int y = 0; y < height; y++)
            for (int x = 0; x < width; x++) out_masks[(size_t)b * px + (size_t)y * width + x] = gfroi::allowed(table.data() + (size_t)b * words, width, x, y) ? 255 : 0;
    return GF_OK;
}

// ---- parameters per sequence (gf_seq_cfg.hpp).  Like the region of interest's setters these run between frames, with the handle's stream drained.
namespace gf {
static int seq_cfg_ready(gf_tracker* h) {   // the first setter of a handle: every sequence's row is the handle's own circle
    if (h->d_seq_disk.p) return GF_OK;
    DevBuf<DiskTable> table; DevBuf<int> md; PinBuf<int> hmd; DevBuf<uint8_t> fb; PinBuf<uint8_t> hfb;
    HIPCHK(table.alloc(h->B)); HIPCHK(md.alloc(h->B)); HIPCHK(hmd.alloc(h->B)); HIPCHK(fb.alloc(h->B)); HIPCHK(hfb.alloc(h->B));
    std::vector<DiskTable> rows((size_t)h->B, h->disk);
    HIPCHK(hipMemcpy(table.p, rows.data(), rows.size() * sizeof(DiskTable), hipMemcpyHostToDevice));
    h->seq_disk = std::move(rows);
    h->d_seq_disk = std::move(table); h->d_seq_md = std::move(md); h->h_seq_md = std::move(hmd); h->d_seq_fb = std::move(fb); h->h_seq_fb = std::move(hfb);
    return GF_OK;
}
// a frame staged by gf_tracker_prefetch_* that lists the sequence: its depth pointers were judged with the parameters in force when it was staged
static bool seq_is_staged(const gf_tracker* h, int seq) {
    for (int k = 0; k < h->pf_count; k++) {
        const std::vector<int>& l = h->pf_seq[(h->pf_head + k) & 1];
        if (std::find(l.begin(), l.end(), seq) != l.end()) return true;
    }
    return false;
}
}  // namespace gf

int gf_tracker_set_seq_cfg(gf_tracker* h, int seq, const gf_tracker_seq_cfg* c) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    if (h->seq[seq].started) return gf::set_err(GF_ERR_INVALID, "sequence %d has taken a frame: its parameters are fixed until gf_tracker_reset_seq", seq);
    if (gf::seq_is_staged(h, seq)) return gf::set_err(GF_ERR_INVALID, "sequence %d is listed by a staged frame: gf_tracker_track_prefetched has to consume it first", seq);
    const gf_tracker_seq_cfg want = c ? *c : gfseq::of_handle(h->cfg);
    char msg[256];
    if (c && !gfseq::fits(h->cfg, want, msg, sizeof msg)) return gf::set_err(GF_ERR_INVALID, "sequence %d: %s", seq, msg);
    if (want.depth_cam && h->stereo_on(seq)) return gf::set_err(GF_ERR_INVALID, "sequence %d is a stereo sequence (gf_tracker_set_seq_stereo): stereo and depth_cam exclude each other", seq);
    if (!c && !h->d_seq_disk.p) return GF_OK;   // nothing to take back: the handle stays one that never set any
    if (int rc = gf::seq_cfg_ready(h)) return rc;
    gf::DiskTable row;
    gf::make_disk_table(want.min_dist, row);
    HIPCHK(hipMemcpy(h->d_seq_disk.p + seq, &row, sizeof row, hipMemcpyHostToDevice));
    h->seq_disk[seq] = row;
    h->par[seq] = want;
    return GF_OK;
}

int gf_tracker_get_seq_cfg(gf_tracker* h, int seq, gf_tracker_seq_cfg* out) {
    if (!h || !out) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    *out = h->par[seq];
    return GF_OK;
}

// ---- a camera model per sequence (gf_camera_models.hpp; readIntrinsicParameter, feature_tracker.cpp:745-759).  Between frames, with the stream drained.
namespace gf {
static int seq_camera_ready(gf_tracker* h) {   // the first setter of a model other than PINHOLE: the cameras by sequence, the list and the two tables of pairs by list position
    if (h->d_cams.p) return GF_OK;
    const size_t B = (size_t)h->B, cap = (size_t)h->cap;
    DevBuf<gfcam::Camera> cams; DevBuf<int> of; PinBuf<int> hof; DevBuf<float2> lk, out; PinBuf<float2> hlk, hout;
    HIPCHK(cams.alloc(B)); HIPCHK(of.alloc(B)); HIPCHK(hof.alloc(B));
    HIPCHK(lk.alloc(B * cap)); HIPCHK(out.alloc(B * cap)); HIPCHK(hlk.alloc(B * cap)); HIPCHK(hout.alloc(B * cap));
    h->cam_on.assign(B, 0); h->cam_model.assign(B, gf_camera_model_ex{}); h->cam.assign(B, gfcam::Camera{});
    h->d_cams = std::move(cams); h->d_cam_of = std::move(of); h->h_cam_of = std::move(hof);
    h->d_un_lk = std::move(lk); h->d_un_out = std::move(out); h->h_un_lk = std::move(hlk); h->h_un_out = std::move(hout);
    return GF_OK;
}
}  // namespace gf

namespace gf {
// both setters behind their checker: `checked` is `m` as gfcam::prepare passed it
static int seq_camera_set(gf_tracker* h, int seq, const gf_camera_model_ex& m, const gfcam::Camera& checked) {
    if (m.model != GF_CAMERA_PINHOLE && m.model != GF_CAMERA_PINHOLE_FULL && !h->dreg_on.empty() && h->dreg_on[seq])
        return gf::set_err(GF_ERR_INVALID, "sequence %d has a depth registration (gf_tracker_set_seq_depth_reg), which projects through a GF_CAMERA_PINHOLE or GF_CAMERA_PINHOLE_FULL only: clear it before a %s camera is set", seq, gfcam::model_name(m.model));
    if (m.model == GF_CAMERA_PINHOLE) {   // the eight camera fields of the sequence's parameters, through their own setter
        gf_tracker_seq_cfg want = h->par[seq];
        want.fx = m.proj[0]; want.fy = m.proj[1]; want.cx = m.proj[2]; want.cy = m.proj[3];
        want.k1 = m.dist[0]; want.k2 = m.dist[1]; want.p1 = m.dist[2]; want.p2 = m.dist[3];
        if (int rc = gf_tracker_set_seq_cfg(h, seq, &want)) return rc;
        if (!h->cam_on.empty()) h->cam_on[seq] = 0;
        return GF_OK;
    }
    if (int rc = gf::seq_camera_ready(h)) return rc;
    HIPCHK(hipMemcpy(h->d_cams.p + seq, &checked, sizeof checked, hipMemcpyHostToDevice));
    h->cam[seq] = checked; h->cam_model[seq] = m; h->cam_on[seq] = 1;
    return GF_OK;
}
static int seq_camera_open(gf_tracker* h, int seq, const void* m) {   // what both setters refuse ahead of the model's own rules
    if (!h || !m) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    if (h->seq[seq].started) return gf::set_err(GF_ERR_INVALID, "sequence %d has taken a frame: its camera is fixed until gf_tracker_reset_seq", seq);
    if (gf::seq_is_staged(h, seq)) return gf::set_err(GF_ERR_INVALID, "sequence %d is listed by a staged frame: gf_tracker_track_prefetched has to consume it first", seq);
    return GF_OK;
}
}  // namespace gf

int gf_tracker_set_seq_camera(gf_tracker* h, int seq, const gf_camera_model* m) {
    if (int rc = gf::seq_camera_open(h, seq, m)) return rc;
    gfcam::Camera checked;
    char msg[320];
    if (!gfcam::prepare(*m, checked, msg, sizeof msg)) return gf::set_err(GF_ERR_INVALID, "sequence %d: %s", seq, msg);
    return gf::seq_camera_set(h, seq, gfcam::widen(*m), checked);
}

int gf_tracker_set_seq_camera_ex(gf_tracker* h, int seq, const gf_camera_model_ex* m) {
    if (int rc = gf::seq_camera_open(h, seq, m)) return rc;
    gfcam::Camera checked;
    char msg[320];
    if (!gfcam::prepare(*m, checked, msg, sizeof msg)) return gf::set_err(GF_ERR_INVALID, "sequence %d: %s", seq, msg);
    return gf::seq_camera_set(h, seq, *m, checked);
}

int gf_tracker_get_camera_lift_stats(gf_tracker* h, long long* launches, long long* sequences) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (launches) *launches = h->lift_launches;
    if (sequences) *sequences = h->lift_sequences;
    return GF_OK;
}

int gf_tracker_get_seq_camera_ex(gf_tracker* h, int seq, gf_camera_model_ex* out) {
    if (!h || !out) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    *out = !h->cam_on.empty() && h->cam_on[seq] ? h->cam_model[seq] : gfcam::widen(gfcam::pinhole_of(h->par[seq]));
    return GF_OK;
}

int gf_tracker_get_seq_camera(gf_tracker* h, int seq, gf_camera_model* out) {
    if (!h || !out) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    if (!h->cam_on.empty() && h->cam_on[seq] && h->cam_model[seq].model > GF_CAMERA_KANNALA_BRANDT)
        return gf::set_err(GF_ERR_INVALID, "sequence %d has a %s camera, which gf_camera_model cannot carry: use gf_tracker_get_seq_camera_ex", seq, gfcam::model_name(h->cam_model[seq].model));
    *out = !h->cam_on.empty() && h->cam_on[seq] ? gfcam::narrow(h->cam_model[seq]) : gfcam::pinhole_of(h->par[seq]);
    return GF_OK;
}

// ---- a pixel format and an equalise switch per sequence (gf_seq_format.hpp; rosNodeTest.cpp:238-261 per camera).  Between frames, with the stream drained.
namespace gf { static int stereo_eq_ready(gf_tracker* h); }
int gf_tracker_set_seq_format(gf_tracker* h, int seq, const gf_tracker_seq_format* f) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    if (h->seq[seq].started) return gf::set_err(GF_ERR_INVALID, "sequence %d has taken a frame: its format is fixed until gf_tracker_reset_seq", seq);
    if (h->pf_count) return gf::set_err(GF_ERR_INVALID, "sequence %d: a frame staged by gf_tracker_prefetch_* is waiting (the staging buffers may have to grow): gf_tracker_track_prefetched has to consume it first", seq);
    const gf_tracker_seq_format own = gfseqfmt::of_handle(h->cfg), want = f ? *f : own;
    const int W = h->cfg.width, H = h->cfg.height, B = h->B;
    char msg[256];
    if (f && !gfseqfmt::fits(gf::seq_width(h, seq), gf::seq_height(h, seq), want, msg, sizeof msg)) return gf::set_err(GF_ERR_INVALID, "sequence %d: %s", seq, msg);   // (rows of the sequence's own width)
    if (h->stereo_on(seq) && want.pixel_format != GF_PIX_MONO8)
        return gf::set_err(GF_ERR_INVALID, "sequence %d is a stereo sequence (gf_tracker_set_seq_stereo): it takes GF_PIX_MONO8 frames only, got pixel format %d", seq, want.pixel_format);
    if (!f && !h->fmt_any) return GF_OK;   // nothing to take back: the handle stays one that never set any
    // what a handle created with that format would have, into locals first: a failed allocation changes nothing
    const size_t px = (size_t)W * H;
    const int ch = std::max(h->raw_ch, gfpix::channels(want.pixel_format));
    gf::DevBuf<uint8_t> cvt, eq, lut, raw, raw2, dmix; gf::PinBuf<uint8_t> hmix;
    const bool need_cvt = want.pixel_format != GF_PIX_MONO8 && !h->d_cvt.p, need_eq = want.equalize && !h->d_eq.p, need_raw = ch > h->raw_ch, need_mix = !h->h_mix.p;
    const size_t mix_bytes = (size_t)B * (3 * sizeof(gf_frame_ref) + sizeof(int));
    if (need_cvt) HIPCHK(cvt.alloc((size_t)B * px));
    if (need_eq) { HIPCHK(eq.alloc((size_t)B * px)); HIPCHK(lut.alloc(gf::clahe_lut_bytes(B, gf::kClaheTiles, gf::kClaheTiles))); }
    if (need_raw) { HIPCHK(raw.alloc((size_t)B * px * ch)); if (h->d_raw2.p) HIPCHK(raw2.alloc((size_t)B * px * ch)); }
    if (need_mix) { HIPCHK(dmix.alloc(mix_bytes)); HIPCHK(hmix.alloc(mix_bytes)); }
    if (need_cvt) h->d_cvt = std::move(cvt);
    if (need_eq) { h->d_eq = std::move(eq); h->d_eq_lut = std::move(lut); }
    if (need_raw) { h->d_raw = std::move(raw); if (h->d_raw2.p) h->d_raw2 = std::move(raw2); h->raw_ch = ch; }   // nothing is staged and the stream is drained: no frame is lost
    if (need_mix) { h->d_mix = std::move(dmix); h->h_mix = std::move(hmix); }
    if (h->stereo_on(seq) && want.equalize) if (int rc = gf::stereo_eq_ready(h)) return rc;   // the node equalises both eyes
    h->fmt[seq] = want;
    h->fmt_any = true;
    return GF_OK;
}

int gf_tracker_get_seq_format(gf_tracker* h, int seq, gf_tracker_seq_format* out) {
    if (!h || !out) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    *out = h->fmt[seq];
    return GF_OK;
}

// ---- a frame size per sequence (gf_seq_size.hpp; `row`, `col` of trackImage, feature_tracker.cpp:108-109).  Between frames, with the stream drained.
namespace gf {
static int seq_size_ready(gf_tracker* h) {   // the first setter that gives a sequence a size of its own: the table of sizes, the per-call tables, the frame table of the depth samples
    if (h->d_size_rows.p) return GF_OK;
    if (int rc = refs_ready(h)) return rc;
    const size_t B = (size_t)h->B, sub = SizeSub::bytes(B);
    DevBuf<SizeRow> rows; DevBuf<uint8_t> of, dsub; PinBuf<uint8_t> hof, hsub;
    HIPCHK(rows.alloc(GF_MAX_SEQ_SIZES)); HIPCHK(of.alloc(B)); HIPCHK(hof.alloc(B)); HIPCHK(dsub.alloc(sub)); HIPCHK(hsub.alloc(sub));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(select_corners_sized_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->select_lds));
    SizeRow own{};
    own.G = h->G; own.w = h->cfg.width; own.h = h->cfg.height;
    HIPCHK(hipMemcpy(rows.p, &own, sizeof own, hipMemcpyHostToDevice));
    h->size_geom[0] = h->G;
    h->d_size_rows = std::move(rows); h->d_size_of = std::move(of); h->h_size_of = std::move(hof); h->d_size_sub = std::move(dsub); h->h_size_sub = std::move(hsub);
    return GF_OK;
}
}  // namespace gf

int gf_tracker_set_seq_size(gf_tracker* h, int seq, int width, int height) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    const int W = h->cfg.width, H = h->cfg.height;
    const bool back = width == 0 && height == 0;
    char msg[256];
    if (!back && !gfsize::limits_ok(W, H, width, height, msg, sizeof msg)) return gf::set_err(GF_ERR_INVALID, "sequence %d: %s", seq, msg);
    if (!back && !gfsize::fits_slot(width, height, W, H)) return gf::set_err(GF_ERR_INVALID, "sequence %d: the pyramid of width %d, height %d does not fit the slot of %d x %d", seq, width, height, W, H);
    const bool own = back || (width == W && height == H);
    if (own && !h->size_any) return GF_OK;   // nothing to take back, whatever the sequence's state: the handle stays one that never set any
    if (h->seq[seq].started) return gf::set_err(GF_ERR_INVALID, "sequence %d has taken a frame: its width and height are fixed until gf_tracker_reset_seq", seq);
    if (gf::seq_is_staged(h, seq)) return gf::set_err(GF_ERR_INVALID, "sequence %d is listed by a staged frame: gf_tracker_track_prefetched has to consume it first (width, height)", seq);
    if (!h->roi_has.empty() && h->roi_has[seq]) return gf::set_err(GF_ERR_INVALID, "sequence %d has a region of interest, an image of its present width and height: clear it first (gf_tracker_set_roi with a null mask)", seq);
    const int r = h->sizes.find(seq, own ? 0 : width, own ? 0 : height);
    if (r < 0) return gf::set_err(GF_ERR_INVALID, "sequence %d: width %d, height %d would be distinct size %d on the handle, GF_MAX_SEQ_SIZES is %d", seq, width, height, GF_MAX_SEQ_SIZES + 1, GF_MAX_SEQ_SIZES);
    if (int rc = gf::seq_size_ready(h)) return rc;
    if (r != 0) {
        gfsize::Geom g;
        gfsize::build_geom(width, height, g);
        gf::SizeRow row{};
        memcpy(&row.G, &g, sizeof g);
        row.w = width; row.h = height;
        HIPCHK(hipMemcpy(h->d_size_rows.p + r, &row, sizeof row, hipMemcpyHostToDevice));
        h->size_geom[r] = row.G;
    }
    h->sizes.move(seq, r, width, height);
    h->size_any = true;
    // The sequence's rows of the region tables were written in the geometry of the size it leaves (a compose writes the words of its own frame alone), and the
    // detector will read them in the new one: the whole rows go back to all ones -- the sequence has no base region here -- whether or not it has boxes, and the
    // boxes, which stay, are clipped to and composed in the new frame.
    if (h->d_roi.p) {
        const size_t off = (size_t)seq * h->roi_words;
        HIPCHK(hipMemsetAsync(h->d_roi.p + off, 0xff, h->roi_words * sizeof(uint32_t), h->stream));
        if (h->d_roi_base.p) HIPCHK(hipMemsetAsync(h->d_roi_base.p + off, 0xff, h->roi_words * sizeof(uint32_t), h->stream));
        if (!h->boxes.empty() && !h->boxes[seq].empty()) { if (int rc = gf::boxes_compose(h, 1, &seq)) return rc; }
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return GF_OK;
}

int gf_tracker_get_seq_size(gf_tracker* h, int seq, int* width, int* height) {
    if (!h || !width || !height) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    const int r = h->sizes.row_of[seq];
    *width = h->sizes.w[r]; *height = h->sizes.h[r];
    return GF_OK;
}

// ---- a depth registration per sequence (gf_depth_reg.hpp; the driver's aligned_depth_to_color, config/realsense/m2dgrp.yaml:23).  Between frames, with the stream drained.
namespace gf {
static int seq_depth_reg_ready(gf_tracker* h) {   // the first setter of a handle: the registered frames and the z-buffer at the handle's capacity, the call's table, the two events
    if (h->d_dreg.p) return GF_OK;
    const size_t B = (size_t)h->B;
    DevBuf<uint16_t> frames; DepthRegStage stage; Event ev[2];
    HIPCHK(frames.alloc(B * h->cfg.width * h->cfg.height));
    if (int rc = depth_reg_fit(stage, B, B * gfdreg::zwords_of(h->cfg.width, h->cfg.height))) return rc;
    for (auto& e : ev) HIPCHK(hipEventCreate(&e.e));
    h->dreg_on.assign(B, 0); h->dreg.assign(B, gf_depth_reg{});
    h->d_dreg = std::move(frames);
    h->dreg_stage.z = std::move(stage.z); h->dreg_stage.d_jobs = std::move(stage.d_jobs); h->dreg_stage.h_jobs = std::move(stage.h_jobs); h->dreg_stage.primed = false;
    for (int i = 0; i < 2; i++) std::swap(h->ev_dreg[i].e, ev[i].e);
    return GF_OK;
}
}  // namespace gf

int gf_tracker_set_seq_depth_reg(gf_tracker* h, int seq, const gf_depth_reg* reg) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    char msg[320];
    if (reg && !gfdreg::check(*reg, msg, sizeof msg)) return gf::set_err(GF_ERR_INVALID, "sequence %d: %s", seq, msg);
    if (reg && h->stereo_on(seq)) return gf::set_err(GF_ERR_INVALID, "sequence %d is a stereo sequence (gf_tracker_set_seq_stereo): stereo and a depth registration exclude each other", seq);
    if (!reg && h->dreg_on.empty()) return GF_OK;   // nothing to take back, whatever the sequence's state: the handle stays one that never set any
    if (h->seq[seq].started) return gf::set_err(GF_ERR_INVALID, "sequence %d has taken a frame: its depth registration is fixed until gf_tracker_reset_seq", seq);
    if (gf::seq_is_staged(h, seq)) return gf::set_err(GF_ERR_INVALID, "sequence %d is listed by a staged frame: gf_tracker_track_prefetched has to consume it first (depth registration)", seq);
    if (reg && !h->cam_on.empty() && h->cam_on[seq] && h->cam_model[seq].model != GF_CAMERA_PINHOLE_FULL)
        return gf::set_err(GF_ERR_INVALID, "sequence %d has a %s camera (gf_tracker_set_seq_camera); depth is registered to a GF_CAMERA_PINHOLE or GF_CAMERA_PINHOLE_FULL only: set one first", seq, gfcam::model_name(h->cam_model[seq].model));
    if (int rc = gf::seq_depth_reg_ready(h)) return rc;
    h->dreg_on[seq] = reg ? 1 : 0;
    h->dreg[seq] = reg ? *reg : gf_depth_reg{};
    return GF_OK;
}

int gf_tracker_get_seq_depth_reg(gf_tracker* h, int seq, gf_depth_reg* out, int* has) {
    if (!h || !has) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    *has = !h->dreg_on.empty() && h->dreg_on[seq] ? 1 : 0;
    if (*has && out) *out = h->dreg[seq];
    return GF_OK;
}

int gf_tracker_get_depth_reg_stats(gf_tracker* h, long long* launches, long long* frames, double* kernel_ms) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (launches) *launches = h->dreg_launches;
    if (frames) *frames = h->dreg_frames;
    if (kernel_ms) *kernel_ms = h->dreg_ms;
    return GF_OK;
}

// ---- rejectWithF per sequence (gf_reject_f.hpp; feature_tracker.cpp:711-743).  Between frames, at any time.
int gf_tracker_set_seq_reject_f(gf_tracker* h, int seq, const gf_reject_f_cfg* c) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    const bool on = c && c->enable;
    char msg[200];
    if (on && !gfrf::check_cfg(c->f_threshold, c->focal_length, msg, sizeof msg)) return gf::set_err(GF_ERR_INVALID, "sequence %d: rejectWithF: %s", seq, msg);
    if (!on && h->rf_on.empty()) return GF_OK;   // nothing to take back: the handle stays one that never set any
    if (gf::seq_is_staged(h, seq)) return gf::set_err(GF_ERR_INVALID, "sequence %d is listed by a staged frame: gf_tracker_track_prefetched has to consume it first (rejectWithF)", seq);
    if (on && h->cap > gfrf::kMaxCandidates) return gf::set_err(GF_ERR_CAPACITY, "sequence %d: rejectWithF takes at most %d points per sequence, the handle holds %d", seq, gfrf::kMaxCandidates, h->cap);
    if (h->rf_on.empty()) {   // the first setter of the handle: the call's table and the events, into locals first
        gf::RejectFStage stage; gf::Event ev[4];
        if (!h->rf_host) {
            if (int rc = gf::reject_f_fit(stage, (size_t)h->B)) return rc;
            for (auto& e : ev) HIPCHK(hipEventCreate(&e.e));
        }
        h->rf_on.assign(h->B, 0); h->rf.assign(h->B, gf_reject_f_cfg{});
        h->rf_stage = std::move(stage);
        for (int i = 0; i < 4; i++) std::swap(h->ev_rf[i].e, ev[i].e);
    }
    h->rf_on[seq] = on ? 1 : 0;
    h->rf[seq] = on ? *c : gf_reject_f_cfg{};
    return GF_OK;
}

int gf_tracker_get_seq_reject_f(gf_tracker* h, int seq, gf_reject_f_cfg* out) {
    if (!h || !out) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    *out = !h->rf_on.empty() && h->rf_on[seq] ? h->rf[seq] : gf_reject_f_cfg{};
    return GF_OK;
}

int gf_tracker_get_reject_f_stats(gf_tracker* h, gf_reject_f_stats* out) {
    if (!h || !out) return gf::set_err(GF_ERR_INVALID, "null argument");
    *out = h->rf_stats;
    return GF_OK;
}

// ---- a right camera per sequence (the stereo branch, feature_tracker.cpp:259-303; gf_stereo_kernels.hpp).  Between frames, with the stream drained.
namespace gf {
static int seq_stereo_ready(gf_tracker* h) {   // the first setter of a handle that turns a switch on: the right pyramids, the table of sizes, the call's tables
    if (h->d_rimg.p) return GF_OK;
    if (int rc = seq_size_ready(h)) return rc;   // the kernel reads a SizeRow per block: the table of sizes (row 0: the handle's own), and with it the frame table
    const size_t B = (size_t)h->B, rows = B * h->cap;
    DevBuf<uint8_t> rimg, dsz, dfb, dst, dfw; PinBuf<uint8_t> hsz, hfb, hst;
    DevBuf<int> dro, dlo, dnt, drw, dcu; PinBuf<int> hro, hlo, hnt, hrw, hcu;
    DevBuf<float2> dpt, dun; PinBuf<float2> hpt, hun; DevBuf<gf_frame_ref> drf; PinBuf<gf_frame_ref> hrf;
    DevBuf<gfcam::Camera> dcm; DevBuf<int> dco, dsn; PinBuf<int> hco;
    HIPCHK(dun.alloc(rows)); HIPCHK(hun.alloc(rows)); HIPCHK(dcm.alloc(B)); HIPCHK(dco.alloc(B)); HIPCHK(dsn.alloc(B)); HIPCHK(hco.alloc(B));
    HIPCHK(rimg.alloc(B * h->G.img_bytes));
    HIPCHK(dsz.alloc(B)); HIPCHK(dfb.alloc(B)); HIPCHK(dst.alloc(rows)); HIPCHK(dfw.alloc(rows)); HIPCHK(hsz.alloc(B)); HIPCHK(hfb.alloc(B)); HIPCHK(hst.alloc(rows));
    HIPCHK(dro.alloc(B)); HIPCHK(dlo.alloc(B)); HIPCHK(dnt.alloc(B)); HIPCHK(drw.alloc(rows)); HIPCHK(dcu.alloc(B));
    HIPCHK(hro.alloc(B)); HIPCHK(hlo.alloc(B)); HIPCHK(hnt.alloc(B)); HIPCHK(hrw.alloc(rows)); HIPCHK(hcu.alloc(B));
    HIPCHK(dpt.alloc(rows)); HIPCHK(hpt.alloc(rows)); HIPCHK(drf.alloc(B)); HIPCHK(hrf.alloc(B));
    h->d_rimg = std::move(rimg); h->d_st_size_of = std::move(dsz); h->d_st_fb = std::move(dfb); h->d_st_status = std::move(dst); h->d_st_fwd = std::move(dfw);
    h->h_st_size_of = std::move(hsz); h->h_st_fb = std::move(hfb); h->h_st_status = std::move(hst);
    h->d_st_right_of = std::move(dro); h->d_st_left_of = std::move(dlo); h->d_st_ntr = std::move(dnt); h->d_st_row = std::move(drw); h->d_st_cur = std::move(dcu);
    h->h_st_right_of = std::move(hro); h->h_st_left_of = std::move(hlo); h->h_st_ntr = std::move(hnt); h->h_st_row = std::move(hrw); h->h_st_cur = std::move(hcu);
    h->d_st_pts = std::move(dpt); h->h_st_pts = std::move(hpt); h->d_st_refs = std::move(drf); h->h_st_refs = std::move(hrf);
    h->d_st_un = std::move(dun); h->h_st_un = std::move(hun); h->d_st_cams = std::move(dcm); h->d_st_cam_of = std::move(dco); h->d_st_n = std::move(dsn); h->h_st_cam_of = std::move(hco);
    h->st_on.assign(B, 0); h->st_cfg.assign(B, gf_stereo_cfg{}); h->st_cam.assign(B, gfcam::Camera{});
    return GF_OK;
}
static int stereo_eq_ready(gf_tracker* h) {   // the first stereo sequence that equalises: the right eye's frames, LUTs and table of sources
    if (h->d_st_eq.p) return GF_OK;
    const size_t B = (size_t)h->B;
    DevBuf<uint8_t> eq, lut; DevBuf<gf_frame_ref> ds; PinBuf<gf_frame_ref> hs;
    HIPCHK(eq.alloc(B * h->cfg.width * h->cfg.height)); HIPCHK(lut.alloc(clahe_lut_bytes((int)B, kClaheTiles, kClaheTiles))); HIPCHK(ds.alloc(B)); HIPCHK(hs.alloc(B));
    h->d_st_eq = std::move(eq); h->d_st_eq_lut = std::move(lut); h->d_st_eqsrc = std::move(ds); h->h_st_eqsrc = std::move(hs);
    return GF_OK;
}
}  // namespace gf

int gf_tracker_set_seq_stereo(gf_tracker* h, int seq, const gf_stereo_cfg* c) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    if (c && c->enable != 0 && c->enable != 1) return gf::set_err(GF_ERR_INVALID, "sequence %d: gf_stereo_cfg.enable must be 0 or 1, got %d", seq, c->enable);
    if (c && c->reserved != 0) return gf::set_err(GF_ERR_INVALID, "sequence %d: gf_stereo_cfg.reserved must be 0, got %d", seq, c->reserved);
    const bool on = c && c->enable;
    gfcam::Camera cam{};
    char msg[320];
    if (on && !gfcam::prepare(c->right, cam, msg, sizeof msg)) return gf::set_err(GF_ERR_INVALID, "sequence %d, right camera: %s", seq, msg);
    if (!on && h->st_on.empty()) return GF_OK;   // nothing to take back, whatever the sequence's state: the handle stays one that never set any
    if (h->seq[seq].started) return gf::set_err(GF_ERR_INVALID, "sequence %d has taken a frame: its right camera is fixed until gf_tracker_reset_seq", seq);
    if (gf::seq_is_staged(h, seq)) return gf::set_err(GF_ERR_INVALID, "sequence %d is listed by a staged frame: gf_tracker_track_prefetched has to consume it first (stereo)", seq);
    if (on && h->par[seq].depth_cam) return gf::set_err(GF_ERR_INVALID, "sequence %d has a depth camera (depth_cam 1): its second image is a depth frame, not a right frame; stereo and depth_cam exclude each other", seq);
    if (on && !h->dreg_on.empty() && h->dreg_on[seq]) return gf::set_err(GF_ERR_INVALID, "sequence %d has a depth registration: stereo and a depth registration exclude each other", seq);
    if (on && h->fmt[seq].pixel_format != GF_PIX_MONO8) return gf::set_err(GF_ERR_INVALID, "sequence %d has pixel format %d: a stereo sequence takes GF_PIX_MONO8 frames only", seq, h->fmt[seq].pixel_format);
    if (int rc = gf::seq_stereo_ready(h)) return rc;
    if (on && h->fmt[seq].equalize) if (int rc = gf::stereo_eq_ready(h)) return rc;
    if (on) HIPCHK(hipMemcpy(h->d_st_cams.p + seq, &cam, sizeof cam, hipMemcpyHostToDevice));
    h->st_on[seq] = on ? 1 : 0;
    h->st_cfg[seq] = on ? *c : gf_stereo_cfg{};
    h->st_cam[seq] = cam;
    if (!on && h->stereo_depth_on(seq)) return gf_tracker_set_seq_stereo_depth(h, seq, nullptr);   // no right camera, no match, no depth
    return GF_OK;
}

// ---- the depth a stereo sequence's matches determine (gf_stereo_depth.hpp; gf_stereo_depth_kernels.hpp).  Between frames, with the stream drained.
namespace gf {
static int seq_stereo_depth_ready(gf_tracker* h) {   // the first setter of a handle that turns a switch on: the table of entries and the call's two output tables
    if (h->d_sd_entries.p) return GF_OK;
    const size_t B = (size_t)h->B, rows = B * h->cap;
    DevBuf<gfsd::Entry> de; PinBuf<gfsd::Entry> he; DevBuf<uint16_t> dm; PinBuf<uint16_t> hm; DevBuf<uint8_t> dw; PinBuf<uint8_t> hw;
    HIPCHK(de.alloc(B)); HIPCHK(he.alloc(B)); HIPCHK(dm.alloc(rows)); HIPCHK(hm.alloc(rows)); HIPCHK(dw.alloc(rows)); HIPCHK(hw.alloc(rows));
    HIPCHK(hipMemset(de.p, 0, B * sizeof(gfsd::Entry)));   // on == 0: a stereo sequence without the switch leaves the kernel at once
    h->d_sd_entries = std::move(de); h->d_sd_mm = std::move(dm); h->h_sd_mm = std::move(hm); h->d_sd_why = std::move(dw); h->h_sd_why = std::move(hw);
    memset(he.p, 0, B * sizeof(gfsd::Entry));
    h->sd_entry = std::move(he);
    h->sd_on.assign(B, 0); h->sd_cfg.assign(B, gf_stereo_depth_cfg{});
    return GF_OK;
}
}  // namespace gf

int gf_tracker_set_seq_stereo_depth(gf_tracker* h, int seq, const gf_stereo_depth_cfg* c) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    if (c && c->enable != 0 && c->enable != 1) return gf::set_err(GF_ERR_INVALID, "sequence %d: gf_stereo_depth_cfg.enable must be 0 or 1, got %d", seq, c->enable);
    if (c && c->right_obs != 0 && c->right_obs != 1) return gf::set_err(GF_ERR_INVALID, "sequence %d: gf_stereo_depth_cfg.right_obs must be 0 or 1, got %d", seq, c->right_obs);
    const bool on = c && c->enable;
    char msg[320];
    if (on && !gfsd::check(*c, msg, sizeof msg)) return gf::set_err(GF_ERR_INVALID, "sequence %d: %s", seq, msg);
    if (!on && h->sd_on.empty()) return GF_OK;   // nothing to take back, whatever the sequence's state: the handle stays one that never set any
    if (h->seq[seq].started) return gf::set_err(GF_ERR_INVALID, "sequence %d has taken a frame: its stereo depth is fixed until gf_tracker_reset_seq", seq);
    if (gf::seq_is_staged(h, seq)) return gf::set_err(GF_ERR_INVALID, "sequence %d is listed by a staged frame: gf_tracker_track_prefetched has to consume it first (stereo depth)", seq);
    if (on && !h->stereo_on(seq)) return gf::set_err(GF_ERR_INVALID, "sequence %d has no right camera: gf_tracker_set_seq_stereo comes first, a depth needs a match (stereo depth)", seq);
    if (int rc = gf::seq_stereo_depth_ready(h)) return rc;
    gfsd::Entry e;   // on == 0
    memset(&e, 0, sizeof e);
    if (on) { e.left = gf::reject_f_camera(h, seq); e.right = h->st_cam[seq]; e.rig = gfsd::rig_of(*c); e.on = 1; }
    HIPCHK(hipMemcpy(h->d_sd_entries.p + seq, &e, sizeof e, hipMemcpyHostToDevice));
    h->sd_entry.p[seq] = e;
    h->sd_on[seq] = on ? 1 : 0;
    h->sd_cfg[seq] = on ? *c : gf_stereo_depth_cfg{};
    return GF_OK;
}

int gf_tracker_get_seq_stereo_depth(gf_tracker* h, int seq, gf_stereo_depth_cfg* out) {
    if (!h || !out) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    *out = h->stereo_depth_on(seq) ? h->sd_cfg[seq] : gf_stereo_depth_cfg{};
    return GF_OK;
}

int gf_tracker_get_stereo_depth_stats(gf_tracker* h, gf_stereo_depth_stats* out) {
    if (!h || !out) return gf::set_err(GF_ERR_INVALID, "null argument");
    *out = h->sd_stats;
    return GF_OK;
}

int gf_tracker_get_seq_stereo(gf_tracker* h, int seq, gf_stereo_cfg* out) {
    if (!h || !out) return gf::set_err(GF_ERR_INVALID, "null argument");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    *out = h->stereo_on(seq) ? h->st_cfg[seq] : gf_stereo_cfg{};
    return GF_OK;
}

int gf_tracker_get_stereo_stats(gf_tracker* h, gf_stereo_stats* out) {
    if (!h || !out) return gf::set_err(GF_ERR_INVALID, "null argument");
    *out = h->st_stats;
    return GF_OK;
}

int gf_tracker_reset_seq(gf_tracker* h, int seq) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    if (gf::seq_is_staged(h, seq)) return gf::set_err(GF_ERR_INVALID, "sequence %d is listed by a staged frame: gf_tracker_track_prefetched has to consume it first", seq);
    const bool show = h->seq[seq].show_track;   // a setting, like the region of interest: it stays; the recorded picture goes
    h->seq[seq] = gf::SeqState{};   // no tracks, no previous frame: LK has nothing to read in the sequence's pyramids, whatever they hold
    h->seq[seq].show_track = show;
    return GF_OK;
}

// ---- the track image (gf_track_draw.hpp; drawTrack / getTrackImage, feature_tracker.cpp:849-905, :1047)
int gf_tracker_set_show_track(gf_tracker* h, int count, const int* seq, int on) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (int rc = gf::check_list(h, count, seq)) return rc;
    if (on && count > 0 && !h->d_draw_prims.p) {   // the first switch of the handle that goes on
        const size_t row = gfdraw::list_capacity(h->cap) + (h->d_roi_base.p ? (size_t)GF_MAX_BOXES_PER_SEQ : 0);   // draw_room(), defined below
        gf::DevBuf<gfdraw::Prim> dp; gf::PinBuf<gfdraw::Prim> hp; gf::DevBuf<gfdraw::DrawJob> dj; gf::PinBuf<gfdraw::DrawJob> hj;
        HIPCHK(dp.alloc((size_t)h->B * row)); HIPCHK(hp.alloc((size_t)h->B * row)); HIPCHK(dj.alloc(h->B)); HIPCHK(hj.alloc(h->B));
        h->d_draw_prims = std::move(dp); h->h_draw_prims = std::move(hp); h->d_draw_jobs = std::move(dj); h->h_draw_jobs = std::move(hj);
    }
    for (int i = 0; i < count; i++) {
        gf::SeqState& s = h->seq[seq[i]];
        s.show_track = on != 0;
        if (!on) { s.draw_have = s.draw_sent = false; s.draw_list.clear(); s.draw_from.clear(); s.draw_why.clear(); }
    }
    return GF_OK;
}

namespace gf {
// the primitives a sequence's row of d_draw_prims holds: a frame's dots and strokes, and on a handle that has boxes their frames
static size_t draw_room(const gf_tracker* h) { return gfdraw::list_capacity(h->cap) + (h->d_roi_base.p ? (size_t)GF_MAX_BOXES_PER_SEQ : 0); }
// everything a picture call refuses, before anything is copied or launched.  dst[i].data is only asked whether it is null.
static int draw_check(gf_tracker* h, int count, const int* seq, const gf_frame_ref* dst) {
    if (int rc = check_list(h, count, seq)) return rc;
    if (count > 0 && !dst) return set_err(GF_ERR_INVALID, "null table of destinations");
    const size_t room = draw_room(h);
    for (int i = 0; i < count; i++) {
        const SeqState& s = h->seq[seq[i]];
        const size_t row_bytes = 3 * (size_t)seq_width(h, seq[i]);   // a picture of the sequence's own size
        if (!s.show_track) return set_err(GF_ERR_INVALID, "list position %d (sequence %d): show_track is off (gf_tracker_set_show_track)", i, seq[i]);
        if (!s.draw_have && !s.draw_why.empty()) return set_err(GF_ERR_INVALID, "list position %d (sequence %d): the list of its last frame was refused: %s", i, seq[i], s.draw_why.c_str());
        if (!s.draw_have) return set_err(GF_ERR_INVALID, "list position %d (sequence %d): no frame recorded since the switch went on, the handle was created or the sequence reset", i, seq[i]);
        if (s.draw_list.size() > room) return set_err(GF_ERR_CAPACITY, "list position %d (sequence %d): %zu primitives > capacity %zu", i, seq[i], s.draw_list.size(), room);
        const gfref::Verdict v = gfref::check(dst[i], row_bytes, false, false);
        if (v != gfref::kOk)
            return set_err(GF_ERR_INVALID, "destination at list position %d (sequence %d): %s (data %p, pitch %zu bytes, a row is %zu bytes)", i, seq[i], gfref::verdict_text(v), dst[i].data, dst[i].pitch, row_bytes);
    }
    return GF_OK;
}
// the checked call: lists that are new since the sequence's last picture go down, then the jobs, one launch, and the host waits
static int draw_run(gf_tracker* h, int count, const int* seq, const gf_frame_ref* dst) {
    const size_t room = draw_room(h);
    // a frame size per sequence: one launch per distinct size of the list over that size's members; the jobs lie in the order of the plan's compact table
    const bool sized = any_has_size(h, count, seq);
    if (sized) gfsize::plan_list(h->size_plan, h->sizes, count, seq);
    for (int k = 0; k < count; k++) {
        const int i = sized ? h->size_plan.member[k] : k;
        const int q = seq[i];
        const LevelGeom g0 = sized ? h->size_geom[h->size_plan.row[i]].lv[0] : h->G.lv[0];
        SeqState& s = h->seq[q];
        if (!s.draw_sent && !s.draw_list.empty()) {
            memcpy(h->h_draw_prims.p + (size_t)q * room, s.draw_list.data(), s.draw_list.size() * sizeof(gfdraw::Prim));
            HIPCHK(hipMemcpyAsync(h->d_draw_prims.p + (size_t)q * room, h->h_draw_prims.p + (size_t)q * room, s.draw_list.size() * sizeof(gfdraw::Prim), hipMemcpyHostToDevice, h->stream));
        }
        // the background: level 0 of the sequence's newest pyramid, the MONO8 image trackImage tracked on (converted, equalised)
        h->h_draw_jobs.p[k] = gfdraw::DrawJob{h->d_img.p + (size_t)(2 * q + s.slot) * h->G.img_bytes + g0.img_off, (size_t)g0.stride,
                                              static_cast<uint8_t*>(const_cast<void*>(dst[i].data)), dst[i].pitch, h->d_draw_prims.p + (size_t)q * room, (int)s.draw_list.size(), 0};
    }
    HIPCHK(hipMemcpyAsync(h->d_draw_jobs.p, h->h_draw_jobs.p, (size_t)count * sizeof(gfdraw::DrawJob), hipMemcpyHostToDevice, h->stream));
    if (sized) {
        const gfsize::Plan& p = h->size_plan;
        for (int g = 0; g < p.n_groups; g++)
            if (int rc = draw_track_launch(h->d_draw_jobs.p + p.group_first[g], p.group_n[g], h->sizes.w[p.group_row[g]], h->sizes.h[p.group_row[g]], h->stream)) return rc;
    } else if (int rc = draw_track_launch(h->d_draw_jobs.p, count, h->cfg.width, h->cfg.height, h->stream)) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));   // the images are complete, and the page-locked tables free for the next call
    for (int i = 0; i < count; i++) h->seq[seq[i]].draw_sent = true;   // only now: a call that failed on the way sends its lists again
    return GF_OK;
}
}  // namespace gf

int gf_tracker_track_image_some_device(gf_tracker* h, int count, const int* seq, const gf_frame_ref* dst) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (int rc = gf::draw_check(h, count, seq, dst)) return rc;
    if (count == 0) return GF_OK;
    return gf::draw_run(h, count, seq, dst);
}

int gf_tracker_track_image(gf_tracker* h, int seq, uint8_t* dst, int stride) {
    if (!h) return gf::set_err(GF_ERR_INVALID, "null handle");
    if (!dst) return gf::set_err(GF_ERR_INVALID, "null destination");
    if (seq < 0 || seq >= h->B) return gf::set_err(GF_ERR_INVALID, "sequence %d of a handle of %d", seq, h->B);
    const int fw = gf::seq_width(h, seq), fh = gf::seq_height(h, seq);   // a picture of the sequence's own size
    const size_t row = 3 * (size_t)fw;
    if (stride < 0 || (size_t)stride < row) return gf::set_err(GF_ERR_INVALID, "a stride of %d bytes is shorter than a row of %d pixels of 3 bytes", stride, fw);
    gf_frame_ref ref{dst, row};   // checked as the caller's; rendered into the handle's staging image
    if (int rc = gf::draw_check(h, 1, &seq, &ref)) return rc;
    HIPCHK(h->d_draw_host.fit(row * fh));
    ref.data = h->d_draw_host.p;
    if (int rc = gf::draw_run(h, 1, &seq, &ref)) return rc;
    HIPCHK(hipMemcpy2D(dst, (size_t)stride, h->d_draw_host.p, row, row, fh, hipMemcpyDeviceToHost));
    return GF_OK;
}

int gf_tracker_remove_outliers(gf_tracker* h, int seq, const int* ids, int n) {
    if (!h || seq < 0 || seq >= h->B || (n > 0 && !ids)) return gf::set_err(GF_ERR_INVALID, "bad argument");
    gf::remove_outliers(h->seq[seq], ids, n);
    return GF_OK;
}

int gf_tracker_get_state(gf_tracker* h, int seq, int* ids, int* track_cnt, float* prev_pts_xy, int cap, int* n) {
    if (!h || seq < 0 || seq >= h->B || !n) return gf::set_err(GF_ERR_INVALID, "bad argument");
    gf::SeqState& s = h->seq[seq];
    *n = (int)s.ids.size();
    if (*n > cap) return gf::set_err(GF_ERR_CAPACITY, "capacity %d < %d", cap, *n);
    for (int i = 0; i < *n; i++) {
        if (ids) ids[i] = s.ids[i];
        if (track_cnt) track_cnt[i] = s.track_cnt[i];
        if (prev_pts_xy) { prev_pts_xy[2 * i] = s.prev_pts[i].x; prev_pts_xy[2 * i + 1] = s.prev_pts[i].y; }
    }
    return GF_OK;
}

int gf_tracker_set_profiling(gf_tracker* h, int enable) { if (!h) return gf::set_err(GF_ERR_INVALID, "null handle"); h->profiling = enable != 0; return GF_OK; }
int gf_tracker_get_stats(gf_tracker* h, gf_tracker_stats* out) { if (!h || !out) return gf::set_err(GF_ERR_INVALID, "null argument"); *out = h->stats; return GF_OK; }
int gf_tracker_reset_stats(gf_tracker* h) { if (!h) return gf::set_err(GF_ERR_INVALID, "null handle"); h->stats = gf_tracker_stats{}; h->dreg_launches = h->dreg_frames = 0; h->dreg_ms = 0; h->lift_launches = h->lift_sequences = 0; h->rf_stats = gf_reject_f_stats{}; h->st_stats = gf_stereo_stats{}; h->sd_stats = gf_stereo_depth_stats{}; return GF_OK; }

// ------------------------------------------------------------------ building blocks for parity tests
static int tmp_handle(int width, int height, int max_cnt, int min_dist, std::unique_ptr<gf_tracker>& own) {
    gf_tracker_cfg c{};
    c.width = width; c.height = height; c.batch = 1; c.max_cnt = max_cnt; c.min_dist = min_dist; c.flow_back = 0; c.depth_cam = 0;
    c.fx = c.fy = 1; c.cx = c.cy = 0;
    gf_tracker* h = nullptr;
    const int rc = gf_tracker_create(&c, &h);
    own.reset(h);
    return rc;
}

int gf_lk_track(const uint8_t* prev, const uint8_t* next, int width, int height, const float* prev_pts, float* next_pts, uint8_t* status, int n,
                int max_level, int use_initial_flow, long long* iterations) {
    if (!prev || !next || !prev_pts || !next_pts || !status || n < 0) return gf::set_err(GF_ERR_INVALID, "bad argument");
    if (n == 0) return GF_OK;
    std::unique_ptr<gf_tracker> own;   // the handle lives for this call
    if (int rc = tmp_handle(width, height, n, 30, own)) return rc;
    gf_tracker* h = own.get();
    const size_t px = (size_t)width * height;
    HIPCHK(hipMemcpyAsync(h->d_raw.p, prev, px, hipMemcpyHostToDevice, h->stream));
    if (int r = gf::launch_pyramid_one(h, h->d_raw.p, 0)) return r;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpyAsync(h->d_raw.p, next, px, hipMemcpyHostToDevice, h->stream));
    if (int r = gf::launch_pyramid_one(h, h->d_raw.p, 1)) return r;   // LK below: new frame in pyramid 1, previous one in pyramid 0
    h->h_npts.p[0] = n;
    for (int i = 0; i < n; i++) {
        h->h_prev_pts.p[i] = make_float2(prev_pts[2 * i], prev_pts[2 * i + 1]);
        h->h_init_pts.p[i] = make_float2(next_pts[2 * i], next_pts[2 * i + 1]);
    }
    HIPCHK(hipMemcpyAsync(h->d_npts.p, h->h_npts.p, sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_prev_pts.p, h->h_prev_pts.p, (size_t)h->cap * sizeof(float2), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_init_pts.p, h->h_init_pts.p, (size_t)h->cap * sizeof(float2), hipMemcpyHostToDevice, h->stream));
    gf::launch_lk(h, 1, gf::lk_args(h, max_level, use_initial_flow ? 1 : 0, 0, 0, nullptr, nullptr));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h->h_cur_pts.p, h->d_cur_pts.p, (size_t)h->cap * sizeof(float2), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(h->h_status.p, h->d_status.p, (size_t)h->cap, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(h->h_counters.p, h->d_counters.p, (size_t)h->cap * 2 * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    long long it = 0;
    for (int i = 0; i < n; i++) {
        next_pts[2 * i] = h->h_cur_pts.p[i].x; next_pts[2 * i + 1] = h->h_cur_pts.p[i].y;
        status[i] = h->h_status.p[i];
        it += h->h_counters.p[2 * i + 1];
    }
    if (iterations) *iterations = it;
    return GF_OK;
}

// ---- the stereo branch's left-to-right LK (feature_tracker.cpp:259-303; gf_stereo_kernels.hpp) on pairs of frames: the building block of the parity tests
namespace gf {
// one launch of stereo_lk_sized_kernel over `count` list positions whose point rows are `cap` long
static int stereo_lk_launch(const SizeRow* rows, const uint8_t* size_of, size_t slot_bytes, const StereoLkArgs& A, int count, hipStream_t stream) {
    if (count < 1 || A.cap < 1) return GF_OK;
    stereo_lk_sized_kernel<<<dim3((A.cap + 3) / 4, count), 256, 0, stream>>>(rows, size_of, slot_bytes, A);
    HIPCHK(hipGetLastError());
    return GF_OK;
}

static int stereo_match_check(const char* who, const void* left, const void* right, int count, const int* first, const float* pts_xy, const uint8_t* flow_back,
                              const float* right_xy, const uint8_t* status, int* most) {
    if (!left || !right || !first || !flow_back) return set_err(GF_ERR_INVALID, "%s: null argument", who);
    if (count < 1) return set_err(GF_ERR_INVALID, "%s: %d pairs (must be >= 1)", who, count);
    if (first[0] != 0) return set_err(GF_ERR_INVALID, "%s: first[0] is %d, not 0", who, first[0]);
    *most = 0;
    for (int b = 0; b < count; b++) {
        const int m = first[b + 1] - first[b];
        if (m < 0) return set_err(GF_ERR_INVALID, "%s: first[%d] = %d is below first[%d] = %d", who, b + 1, first[b + 1], b, first[b]);
        *most = std::max(*most, m);
    }
    if (first[count] > 0 && (!pts_xy || !right_xy || !status)) return set_err(GF_ERR_INVALID, "%s: null point table", who);
    return GF_OK;
}

// d_left, d_right: `count` tight MONO8 frames each, on the device.  A handle of `count` sequences lives for the call: pair b's left frame goes to pyramid 2 b,
// its right frame to pyramid 2 b + 1, by the route a frame of that size takes in the tracker.  The points go through both of the kernel's sources, as a tracker
// call's do: the first half of a pair's list as rows of LK's table (stored there in reverse order, so that the gather moves every one), the rest as new corners.
static int stereo_match_run(const uint8_t* d_left, const uint8_t* d_right, int count, int width, int height, const int* first, const float* pts_xy, const uint8_t* flow_back,
                            float* right_xy, uint8_t* status, uint8_t* fwd_status, int most) {
    gf_tracker_cfg c{};
    c.width = width; c.height = height; c.batch = count; c.max_cnt = std::max(most, 1); c.min_dist = 30; c.fx = c.fy = 1;
    gf_tracker* raw = nullptr;
    if (int rc = gf_tracker_create(&c, &raw)) return rc;
    std::unique_ptr<gf_tracker> own(raw);   // the handle lives for this call
    gf_tracker* h = raw;
    const int cap = h->cap;
    const size_t rows_n = (size_t)count * cap;
    DevBuf<SizeRow> d_rows; DevBuf<uint8_t> d_size_of; DevBuf<int> d_row; DevBuf<float2> d_right_pts; PinBuf<int> h_row; PinBuf<float2> h_right_pts;
    HIPCHK(d_rows.alloc(1)); HIPCHK(d_size_of.alloc(count)); HIPCHK(d_row.alloc(rows_n)); HIPCHK(d_right_pts.alloc(rows_n)); HIPCHK(h_row.alloc(rows_n)); HIPCHK(h_right_pts.alloc(rows_n));
    SizeRow sr{};
    sr.G = h->G; sr.w = width; sr.h = height;
    HIPCHK(hipMemcpy(d_rows.p, &sr, sizeof sr, hipMemcpyHostToDevice));
    for (int b = 0; b < count; b++) {
        const int n = first[b + 1] - first[b], nt = n / 2;
        h->h_cur.p[b] = 2 * b; h->h_det.p[b] = 2 * b + 1;
        h->h_npts.p[b] = nt; h->h_out_n.p[b] = n - nt;
        h->h_seqmask.p[b] = flow_back[b] ? 1 : 0;
        const float* p = pts_xy + 2 * (size_t)first[b];
        for (int k = 0; k < nt; k++) { h_row.p[(size_t)b * cap + k] = nt - 1 - k; h->h_cur_pts.p[(size_t)b * cap + (nt - 1 - k)] = make_float2(p[2 * k], p[2 * k + 1]); }
        for (int k = nt; k < n; k++) h->h_out_pts.p[(size_t)b * cap + (k - nt)] = make_float2(p[2 * k], p[2 * k + 1]);
    }
    HIPCHK(hipMemcpyAsync(h->d_cur.p, h->h_cur.p, count * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_det.p, h->h_det.p, count * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_npts.p, h->h_npts.p, count * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_out_n.p, h->h_out_n.p, count * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_seqmask.p, h->h_seqmask.p, count, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_row.p, h_row.p, rows_n * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_cur_pts.p, h->h_cur_pts.p, rows_n * sizeof(float2), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_out_pts.p, h->h_out_pts.p, rows_n * sizeof(float2), hipMemcpyHostToDevice, h->stream));
    if (int rc = launch_pyramid(h, d_left, count, h->d_cur.p)) return rc;
    if (int rc = launch_pyramid(h, d_right, count, h->d_det.p)) return rc;
    StereoLkArgs A{};
    A.left = h->d_img.p; A.left_of = h->d_cur.p; A.right = h->d_img.p; A.right_of = h->d_det.p; A.cap = cap;
    A.n_tracked = h->d_npts.p; A.row = d_row.p; A.lk_pts = h->d_cur_pts.p; A.n_new = h->d_out_n.p; A.new_pts = h->d_out_pts.p;
    A.flow_back_of = h->d_seqmask.p; A.right_pts = d_right_pts.p; A.status = h->d_status.p; A.fwd_status = h->d_fwd_status.p;
    if (int rc = stereo_lk_launch(d_rows.p, d_size_of.p, h->G.img_bytes, A, count, h->stream)) return rc;
    HIPCHK(hipMemcpyAsync(h_right_pts.p, d_right_pts.p, rows_n * sizeof(float2), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(h->h_status.p, h->d_status.p, rows_n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(h->h_fwd_status.p, h->d_fwd_status.p, rows_n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int b = 0; b < count; b++)
        for (int k = 0, n = first[b + 1] - first[b]; k < n; k++) {
            const size_t at = (size_t)b * cap + k, o = (size_t)first[b] + k;
            right_xy[2 * o] = h_right_pts.p[at].x; right_xy[2 * o + 1] = h_right_pts.p[at].y;
            status[o] = h->h_status.p[at];
            if (fwd_status) fwd_status[o] = h->h_fwd_status.p[at];
        }
    return GF_OK;
}
}  // namespace gf

int gf_stereo_match_batch_device(const void* d_left, const void* d_right, int count, int width, int height, const int* first, const float* pts_xy, const uint8_t* flow_back,
                                 float* right_xy, uint8_t* status, uint8_t* fwd_status) {
    int most = 0;
    if (int rc = gf::stereo_match_check("gf_stereo_match_batch_device", d_left, d_right, count, first, pts_xy, flow_back, right_xy, status, &most)) return rc;
    if ((reinterpret_cast<uintptr_t>(d_left) | reinterpret_cast<uintptr_t>(d_right)) & 3)
        return gf::set_err(GF_ERR_INVALID, "gf_stereo_match_batch_device: frames at %p and %p, not on 4-byte boundaries", d_left, d_right);
    return gf::stereo_match_run(static_cast<const uint8_t*>(d_left), static_cast<const uint8_t*>(d_right), count, width, height, first, pts_xy, flow_back, right_xy, status, fwd_status, most);
}

int gf_stereo_match_batch(const uint8_t* left, const uint8_t* right, int count, int width, int height, const int* first, const float* pts_xy, const uint8_t* flow_back,
                          float* right_xy, uint8_t* status, uint8_t* fwd_status) {
    int most = 0;
    if (int rc = gf::stereo_match_check("gf_stereo_match_batch", left, right, count, first, pts_xy, flow_back, right_xy, status, &most)) return rc;
    if (width < 1 || height < 1) return gf::set_err(GF_ERR_INVALID, "gf_stereo_match_batch: width %d, height %d", width, height);
    if (int rc = gf::require_device()) return rc;
    const size_t bytes = (size_t)count * width * height;
    gf::DevBuf<uint8_t> dl, dr;
    HIPCHK(dl.fit(bytes)); HIPCHK(dr.fit(bytes));
    HIPCHK(hipMemcpy(dl.p, left, bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dr.p, right, bytes, hipMemcpyHostToDevice));
    return gf::stereo_match_run(dl.p, dr.p, count, width, height, first, pts_xy, flow_back, right_xy, status, fwd_status, most);
}

int gf_pyramid_level(const uint8_t* img, int width, int height, int level, uint8_t* out, int16_t* deriv_xy) {
    if (!img || level < 0) return gf::set_err(GF_ERR_INVALID, "bad argument");
    std::unique_ptr<gf_tracker> own;   // the handle lives for this call
    if (int rc = tmp_handle(width, height, 4, 30, own)) return rc;
    gf_tracker* h = own.get();
    if (level >= h->G.nlevels) return gf::set_err(GF_ERR_INVALID, "level %d not built (pyramid has %d levels)", level, h->G.nlevels);
    HIPCHK(hipMemcpyAsync(h->d_raw.p, img, (size_t)width * height, hipMemcpyHostToDevice, h->stream));
    if (int r = gf::launch_pyramid_one(h, h->d_raw.p, 0)) return r;
    HIPCHK(hipStreamSynchronize(h->stream));
    const gf::LevelGeom g = h->G.lv[level];
    if (out) HIPCHK(hipMemcpy2D(out, g.w, h->d_img.p + g.img_off, g.stride, g.w, g.h, hipMemcpyDeviceToHost));
    if (deriv_xy) {   // the derivative as lk_solve evaluates it (deriv_probe_kernel calls the same device functions)
        gf::DevBuf<int> d;
        HIPCHK(d.alloc((size_t)g.w * g.h));
        gf::deriv_probe_kernel<<<dim3((((g.w + 7) >> 3) * g.h + 255) / 256), 256, 0, h->stream>>>(h->d_img.p, g, d.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(deriv_xy, d.p, (size_t)g.w * g.h * 4, hipMemcpyDeviceToHost));
    }
    return GF_OK;
}

int gf_min_eigen_val(const uint8_t* img, int width, int height, float* eig) {
    if (!img || !eig) return gf::set_err(GF_ERR_INVALID, "bad argument");
    std::unique_ptr<gf_tracker> own;   // the handle lives for this call
    if (int rc = tmp_handle(width, height, 4, 30, own)) return rc;
    gf_tracker* h = own.get();
    HIPCHK(hipMemcpyAsync(h->d_raw.p, img, (size_t)width * height, hipMemcpyHostToDevice, h->stream));
    if (int r = gf::launch_pyramid_one(h, h->d_raw.p, 0)) return r;
    gf::min_eig_kernel<<<dim3((width + 31) / 32, (height + 7) / 8, 1), 256, 0, h->stream>>>(h->d_img.p, 2 * h->G.img_bytes, h->G.lv[0], h->d_eig.p, h->eig_stride);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(eig, h->d_eig.p, (size_t)width * height * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return GF_OK;
}

int gf_good_features(const uint8_t* img, int width, int height, const uint8_t* mask, int max_corners, int min_dist, float* corners_xy, int* n_out) {
    if (!img || !corners_xy || !n_out || max_corners < 1) return gf::set_err(GF_ERR_INVALID, "bad argument");
    std::unique_ptr<gf_tracker> own;   // the handle lives for this call
    if (int rc = tmp_handle(width, height, max_corners, min_dist, own)) return rc;
    gf_tracker* h = own.get();
    const int W = width, H = height;
    HIPCHK(hipMemcpyAsync(h->d_raw.p, img, (size_t)W * H, hipMemcpyHostToDevice, h->stream));
    if (int r = gf::launch_pyramid_one(h, h->d_raw.p, 0)) return r;
    if (mask) HIPCHK(hipMemcpyAsync(h->d_mask.p, mask, (size_t)W * H, hipMemcpyHostToDevice, h->stream));
    else HIPCHK(hipMemsetAsync(h->d_mask.p, 255, (size_t)W * H, h->stream));
    h->h_want.p[0] = max_corners;
    HIPCHK(hipMemcpyAsync(h->d_want.p, h->h_want.p, sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->d_maxkey.p, 0, sizeof(unsigned), h->stream));
    HIPCHK(hipMemsetAsync(h->d_cand_count.p, 0, sizeof(int), h->stream));
    gf::DetectArgs D = gf::detect_args(h);
    D.frame_of = h->d_cur.p;   // pyramid 0, written above; max_corners >= 1
    D.mask = h->d_mask.p; D.mask_seq_stride = h->mask_stride; D.centers = nullptr; D.n_centers = nullptr;
    gf::launch_detect(h, 1, D);
    gf::SelectArgs S = gf::select_args(h, nullptr, 0);
    S.min_dist = min_dist;
    gf::launch_select<false>(h, 1, S, false, true);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h->h_out_n.p, h->d_out_n.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(h->h_out_pts.p, h->d_out_pts.p, (size_t)h->cap * sizeof(float2), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *n_out = h->h_out_n.p[0];
    for (int i = 0; i < *n_out; i++) { corners_xy[2 * i] = h->h_out_pts.p[i].x; corners_xy[2 * i + 1] = h->h_out_pts.p[i].y; }
    return GF_OK;
}


// ---- calibration of the rocprofv3 FETCH_SIZE counter for the front end's access patterns (profiling aid, scripts/pmc_collect.sh).
// Known byte counts over a buffer far larger than the Infinity Cache, three patterns:
//   mode 0  streaming: every lane reads 16 contiguous bytes (the pattern MI355X_MICROARCH.md calibrates: FETCH_SIZE = 1/2 of the bytes)
//   mode 1  LK tile, aligned: a wavefront reads a 32 x 32 u8 tile, two 16-byte lanes per row (the refill of lk_solve), every 32-byte row segment
//           inside its own 64-byte line, tiles disjoint
//   mode 2  LK tile at an odd 4-byte phase: every row segment straddles two 64-byte lines
namespace gf {
__global__ void __launch_bounds__(256) calib_stream_kernel(const uint4* __restrict__ src, size_t n16, unsigned* __restrict__ sink) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned acc = 0;
    for (; i < n16; i += (size_t)gridDim.x * blockDim.x) { const uint4 v = src[i]; acc += v.x ^ v.y ^ v.z ^ v.w; }
    if (acc == 0x12345678u) sink[0] = acc;
}
__global__ void __launch_bounds__(256) calib_tile_kernel(const uint8_t* __restrict__ src, size_t row_stride, int tiles_per_row, size_t n_tiles, int phase, unsigned* __restrict__ sink) {
    const size_t t = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= n_tiles) return;
    const int lane = threadIdx.x & 63, trow = lane >> 1, thalf = lane & 1;
    const size_t ty = t / tiles_per_row, tx = t % tiles_per_row;
    const uint8_t* p = src + (ty * 32 + trow) * row_stride + tx * 128 + phase + thalf * 16;
    const U4a v = *reinterpret_cast<const U4a*>(p);
    if ((v.x ^ v.y ^ v.z ^ v.w) == 0x12345678u) sink[0] = v.x;
}
}  // namespace gf
int gf_calib_fetch(int mode, size_t buffer_bytes, double* requested_bytes, double* lines64, double* ms) {
    if (mode < 0 || mode > 2 || buffer_bytes < (1u << 20)) return gf::set_err(GF_ERR_INVALID, "bad argument");
    gf::DevBuf<uint8_t> dbuf; gf::DevBuf<unsigned> dsink;
    HIPCHK(dbuf.fit(buffer_bytes)); HIPCHK(dsink.fit(16));
    uint8_t* buf = dbuf.p; unsigned* sink = dsink.p;
    (void)hipMemset(buf, 1, buffer_bytes); (void)hipMemset(sink, 0, 64);
    gf::Event e0, e1; HIPCHK(hipEventCreate(&e0.e)); HIPCHK(hipEventCreate(&e1.e));
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0, 0);
    if (mode == 0) {
        const size_t n16 = buffer_bytes / 16;
        gf::calib_stream_kernel<<<dim3(256 * 8), 256>>>(reinterpret_cast<const uint4*>(buf), n16, sink);
        if (requested_bytes) *requested_bytes = (double)n16 * 16; if (lines64) *lines64 = (double)n16 / 4;
    } else {
        const size_t row_stride = 1u << 16;                 // a 64 KiB wide "image": 512 tile columns of 128 bytes
        const int tiles_per_row = 511;
        const size_t tile_rows = buffer_bytes / row_stride / 32, n_tiles = tile_rows * tiles_per_row;
        const int phase = mode == 1 ? 0 : 44;                // 44: bytes 44..75 of the 128-byte slot -> both halves of the segment in different 64-byte lines
        gf::calib_tile_kernel<<<dim3((unsigned)((n_tiles + 3) / 4)), 256>>>(buf, row_stride, tiles_per_row, n_tiles, phase, sink);
        if (requested_bytes) *requested_bytes = (double)n_tiles * 1024; if (lines64) *lines64 = (double)n_tiles * 32 * (mode == 1 ? 1 : 2);
    }
    (void)hipEventRecord(e1, 0);
    const hipError_t err = hipDeviceSynchronize();
    float t = 0; (void)hipEventElapsedTime(&t, e0, e1);
    if (ms) *ms = t;
    if (err != hipSuccess) return gf::set_err(GF_ERR_HIP, "calibration kernel failed: %s", hipGetErrorString(err));
    return GF_OK;
}

}  // extern "C"
