// feature_tracker.h — C++ host mirror of the reference's FeatureTracker call surface
// (vins_estimator/src/featureTracker/feature_tracker.h:43-99) on top of the C-ABI of libgroundfusion_hip.so.
//
// Same member names, argument meaning and return type as the reference, so that Estimator::inputImage
// (estimator.cpp:213-240) and the ROS plumbing compile against it unchanged once cv::Mat / Eigen are present:
//   * build with -DGF_WITH_OPENCV to take cv::Mat arguments directly (CV_8UC1 image, or CV_8UC3 / CV_8UC4 with a stated channel order; CV_16UC1 depth);
//   * build with -DGF_WITH_EIGEN to return Eigen::Matrix<double,8,1> observations;
//   * without them (this container has neither) the light gf::Image view and std::array<double,8> stand in.
// Errors: the reference logs and carries on; here a failing C-ABI call throws std::runtime_error with gf_last_error().
#pragma once
#include <array>
#include <fstream>
#include <map>
#include <set>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/groundfusion_hip.h"
#ifdef GF_WITH_OPENCV
#include <opencv2/core.hpp>
#endif
#ifdef GF_WITH_EIGEN
#include <eigen3/Eigen/Dense>
#endif

namespace gf {

template <class T> struct ImageView {  // stands in for cv::Mat when OpenCV is absent
    const T* data = nullptr; int rows = 0, cols = 0, stride = 0;  // stride in elements
    // GF_PIX_* of a u8 image (rosNodeTest.cpp:238-254, what getImageFromMsg accepts): a colour image holds cols x 3 or 4 bytes per row, a YUV 4:2:2 or MONO16
    // (little-endian) image cols x 2, a Bayer mosaic cols; `stride` is its row step in bytes, and the tracker converts it to MONO8 on the device as the node's
    // cv_bridge::toCvCopy(msg, MONO8) does on the host
    int pixel_format = GF_PIX_MONO8;
    bool empty() const { return data == nullptr; }
};
typedef ImageView<uint8_t> GrayImage;
typedef ImageView<uint16_t> DepthImage;

#ifdef GF_WITH_EIGEN
typedef Eigen::Matrix<double, 8, 1> Obs8;
typedef Eigen::Vector3d Vec3;
#else
typedef std::array<double, 8> Obs8;
typedef std::array<double, 3> Vec3;
#endif
typedef std::map<int, std::vector<std::pair<int, Obs8>>> FeatureFrame;

class FeatureTracker {
  public:
    // globals of parameters.h the tracker reads: MAX_CNT, MIN_DIST, FLOW_BACK (config/realsense/m2dgrp.yaml:131-136)
    int MAX_CNT = 150, MIN_DIST = 30, FLOW_BACK = 1;
    int row = 0, col = 0;
    bool stereo_cam = false, depth_cam = false;
    std::vector<int> ids, track_cnt;          // refreshed after every trackImage (feature_tracker.h:85-86)
    std::vector<std::pair<float, float>> prev_pts;
    int n_id = 0;

    FeatureTracker() {}
    ~FeatureTracker() { if (h_) gf_tracker_destroy(h_); }
    FeatureTracker(const FeatureTracker&) = delete;
    FeatureTracker& operator=(const FeatureTracker&) = delete;

    // a camodocal calibration file as CameraFactory::generateCameraFromYamlFile takes it (feature_tracker.cpp:745-759): any of its five models
    // (gf_camera_from_yaml_ex); `depth` = depth camera flag
    void readIntrinsicParameter(const std::vector<std::string>& calib_file, const int depth) {
        if (calib_file.empty()) throw std::runtime_error("readIntrinsicParameter: no calibration file");
        if (h_) throw std::runtime_error("readIntrinsicParameter: call it before the first trackImage");
        check(gf_camera_from_yaml_ex(calib_file[0].c_str(), &camera_));
        std::ifstream f(calib_file[0]);   // image_width / image_height are no part of a camera model
        std::string line;
        while (std::getline(f, line)) {
            std::istringstream ss(line);
            std::string key;
            ss >> key;
            double v;
            if (!(ss >> v)) continue;
            if (key == "image_width:") col = (int)v; else if (key == "image_height:") row = (int)v;
        }
        fx_ = camera_.proj[0]; fy_ = camera_.proj[1]; cx_ = camera_.proj[2]; cy_ = camera_.proj[3];
        if (camera_.model == GF_CAMERA_SCARAMUZZA) { fx_ = fy_ = 1.0; cx_ = camera_.affine[3]; cy_ = camera_.affine[4]; }   // no focal length: a valid placeholder
        const bool pin = camera_.model == GF_CAMERA_PINHOLE;   // another model: the handle's own pinhole is a valid placeholder that nothing reads
        k1_ = pin ? camera_.dist[0] : 0; k2_ = pin ? camera_.dist[1] : 0; p1_ = pin ? camera_.dist[2] : 0; p2_ = pin ? camera_.dist[3] : 0;
        depth_cam = depth != 0;
        if (calib_file.size() == 2) {   // the right camera (m_camera[1], feature_tracker.cpp:751-752): the stereo branch, gf_tracker_set_seq_stereo
            stereo_ = gf_stereo_cfg{};
            check(gf_camera_from_yaml_ex(calib_file[1].c_str(), &stereo_.right));
            stereo_.enable = 1;
            stereo_cam = true;
        }
    }
    // two calibration files plus the rig between the eyes: a stereo tracker whose LEFT observations carry the depth its matches determine in their eighth field
    // (gf_tracker_set_seq_stereo_depth; DESIGN.md section 4, "Stereo depth").  rig: R, t with p_left = R p_right + t, the gates, right_obs
    // (gf_stereo_depth_from_yaml reads one from a config file)
    void readIntrinsicParameter(const std::vector<std::string>& calib_file, const int depth, const gf_stereo_depth_cfg& rig) {
        if (calib_file.size() != 2) throw std::runtime_error("readIntrinsicParameter: a rig needs the calibration files of both eyes");
        readIntrinsicParameter(calib_file, depth);
        setStereoDepth(rig);
    }
    // the same switch on its own: before the first trackImage, for a tracker that has a right camera (readIntrinsicParameter with two files)
    void setStereoDepth(const gf_stereo_depth_cfg& rig) {
        if (!stereo_cam) throw std::runtime_error("setStereoDepth: the tracker has no right camera (readIntrinsicParameter with two files comes first)");
        if (h_) check(gf_tracker_set_seq_stereo_depth(h_, 0, &rig));
        stereo_depth_ = rig;
    }
    void setIntrinsics(int width, int height, double fx, double fy, double cx, double cy, double k1 = 0, double k2 = 0, double p1 = 0, double p2 = 0) {
        col = width; row = height; fx_ = fx; fy_ = fy; cx_ = cx; cy_ = cy; k1_ = k1; k2_ = k2; p1_ = p1; p2_ = p2;
        camera_ = gf_camera_model_ex{};
    }
    // EQUALIZE (rosNodeTest.cpp:256-261): the reference's node runs cv::createCLAHE()->apply on every frame before trackImage; the FeatureTracker class itself
    // never does, so it stays off unless asked for.  On: the same CLAHE (clip 40, 8 x 8 tiles) runs on the device ahead of the pyramid.  Before the first frame.
    void setEqualize(bool on) {
        if (h_) throw std::runtime_error("setEqualize: call it before the first trackImage");
        equalize_ = on;
    }

    // The region of interest: the image setMask() (feature_tracker.cpp:56-83, private there as here) starts from instead of an all-255 one -- VINS-Mono's
    // fisheye_mask, which the reference dropped (feature_tracker.cpp:58).  rows x cols bytes of the frame size, `stride` bytes from row to row, non-zero =
    // allowed; nullptr clears.  Tracks that end up on an excluded pixel are dropped in setMask's walk and new corners are sought inside it only
    // (gf_tracker_set_roi).  Any time: it holds from the next trackImage on, and may be replaced between any two frames.  Before the first frame the size must
    // be known (readIntrinsicParameter / setIntrinsics).
    void setRegionOfInterest(const uint8_t* mask, int stride) {
        if (!mask && !h_) { roi_.clear(); return; }
        if (!h_) {   // kept until the handle exists (the first frame decides the pixel format)
            if (!row || !col) throw std::runtime_error("setRegionOfInterest: the frame size is not known yet (readIntrinsicParameter / setIntrinsics)");
            if (stride < col) throw std::runtime_error("setRegionOfInterest: stride < width");
            roi_.resize((size_t)row * col);
            for (int y = 0; y < row; y++) for (int x = 0; x < col; x++) roi_[(size_t)y * col + x] = mask[(size_t)y * stride + x];
            return;
        }
        check(gf_tracker_set_roi(h_, 0, mask, stride));
    }
    // The exclusion boxes of the next frames: what trackImagebox (feature_tracker.cpp:374) takes as darknet's BoundingBoxes, here part of the region setMask()
    // starts from (gf_tracker_set_boxes_some): tracks that end up inside a box are dropped, corners are sought outside.  They hold until replaced; n == 0
    // clears.  Any time; before the first frame they are kept until the handle exists.
    void setBoxes(const gf_box* boxes, int n) {
        if (n < 0 || n > GF_MAX_BOXES_PER_SEQ || (n > 0 && !boxes)) throw std::runtime_error("setBoxes: 0 .. GF_MAX_BOXES_PER_SEQ boxes");
        if (!h_) { boxes_.assign(boxes, boxes + n); return; }
        const int seq = 0, first[2] = {0, n};
        check(gf_tracker_set_boxes_some(h_, 1, &seq, first, boxes));
    }
#ifdef GF_WITH_OPENCV
    void setRegionOfInterest(const cv::Mat& mask) {   // CV_8UC1 of the frame size; an empty Mat clears
        if (mask.empty()) { setRegionOfInterest(nullptr, 0); return; }
        if (mask.type() != CV_8UC1 || (row && (mask.rows != row || mask.cols != col))) throw std::runtime_error("setRegionOfInterest: the mask must be CV_8UC1 of the frame size");
        if (!row) { row = mask.rows; col = mask.cols; }
        setRegionOfInterest(mask.ptr<uint8_t>(), (int)mask.step);
    }
#endif

    // The depth camera's raw stream registered to the colour camera on the device (gf_tracker_set_seq_depth_reg) in the place of the driver's
    // aligned_depth_to_color (config/realsense/m2dgrp.yaml:23): with a registration set, the depth image of trackImage(double, const gf_frame_ref&, ...) is the
    // RAW frame of the depth camera, reg.height rows of reg.width counts, and the host-image forms of trackImage refuse a depth image.  seq: this class holds one
    // sequence, 0.  Before the first trackImage or after it, under the library's rules for the setter (refused once a frame was taken; the camera must be a PINHOLE).
    void setDepthRegistration(int seq, const gf_depth_reg& reg) {
        if (seq != 0) throw std::runtime_error("setDepthRegistration: a FeatureTracker holds one sequence, 0");
        if (h_) check(gf_tracker_set_seq_depth_reg(h_, 0, &reg));
        depth_reg_ = reg; has_depth_reg_ = true;
    }
    void clearDepthRegistration(int seq) {
        if (seq != 0) throw std::runtime_error("clearDepthRegistration: a FeatureTracker holds one sequence, 0");
        if (h_) check(gf_tracker_set_seq_depth_reg(h_, 0, nullptr));
        has_depth_reg_ = false;
    }

    // SHOW_TRACK (parameters.cpp:202; feature_tracker.cpp:304-305): on, every trackImage leaves the picture getTrackImage returns (gf_tracker_set_show_track).
    // Any time; the first frame after it went on already gives a complete picture.
    void setShowTrack(bool on) {
        show_track_ = on;
        const int seq = 0;
        if (h_) check(gf_tracker_set_show_track(h_, 1, &seq, on ? 1 : 0));
    }
    // rejectWithF (feature_tracker.cpp:711-743), which the reference leaves commented out at :183 and :454: on, every trackImage drops the points LK kept that
    // lie further than F_THRESHOLD virtual pixels (parameters.cpp:201) from the epipolar line of the best of 512 eight-point models
    // (gf_tracker_set_seq_reject_f; the definition is this library's).  Any time between frames.
    void setRejectWithF(bool on, double F_THRESHOLD = 1.0) {
        reject_f_ = gf_reject_f_cfg{};
        reject_f_.enable = on ? 1 : 0; reject_f_.f_threshold = F_THRESHOLD;
        if (h_) check(gf_tracker_set_seq_reject_f(h_, 0, on ? &reject_f_ : nullptr));
    }
    // getTrackImage (feature_tracker.cpp:1047; drawTrack :849-905): the frame of the last trackImage with a dot per feature, coloured from blue to red by track
    // length, and a green arrow back to where the feature was one frame earlier -- rows x cols x 3 bytes in the reference's channel order (bgr8), rendered on
    // the device (gf_tracker_track_image).  Without OpenCV: into `store`, with `view` describing it (stride 3 x cols bytes, GF_PIX_BGR8).
    void getTrackImage(std::vector<uint8_t>& store, ImageView<uint8_t>& view) {
        if (!h_) throw std::runtime_error("getTrackImage: no frame yet");
        store.resize((size_t)row * col * 3);
        check(gf_tracker_track_image(h_, 0, store.data(), 3 * col));
        view.data = store.data(); view.rows = row; view.cols = col; view.stride = 3 * col; view.pixel_format = GF_PIX_BGR8;
    }
#ifdef GF_WITH_OPENCV
    cv::Mat getTrackImage() {
        if (!h_) throw std::runtime_error("getTrackImage: no frame yet");
        cv::Mat m(row, col, CV_8UC3);
        check(gf_tracker_track_image(h_, 0, m.ptr<uint8_t>(), (int)m.step));
        return m;
    }
#endif

    FeatureFrame trackImage(double _cur_time, const GrayImage& _img, const DepthImage& _img1 = DepthImage()) {
        if (!h_) { pixel_format_ = _img.pixel_format; create(_img.cols, _img.rows); }
        // one handle has one format (a camera does not change its encoding): the first frame decides, as it decides the size
        if (_img.pixel_format != pixel_format_) throw std::runtime_error("trackImage: the image's pixel format differs from the first frame's");
        if (stereo_cam && !_img1.empty())
            throw std::runtime_error("trackImage: a stereo tracker takes its right image where it lies on the device, trackImage(double, const gf_frame_ref&, const gf_frame_ref&); "
                                     "a host image pair is not served (without a second image the frame is tracked as a mono frame)");
        std::vector<gf_feature_obs> out((size_t)((MAX_CNT + 3) & ~3));
        int n = 0;
        check(gf_tracker_track(h_, 0, _cur_time, _img.data, _img.stride, _img1.empty() ? nullptr : _img1.data, _img1.stride, out.data(), (int)out.size(), &n));
        FeatureFrame featureFrame;
        for (int i = 0; i < n; i++) {
            Obs8 o;
            for (int k = 0; k < 8; k++) o[k] = out[i].v[k];
            featureFrame[out[i].id].emplace_back(out[i].camera_id, o);
        }
        refresh();
        return featureFrame;
    }
    // The same frame where it already lives on the device (gf_tracker_track_some_device_refs): _img = device pointer of row 0 and bytes from row to row of a
    // row x col image in pixel_format (any alignment: the luma plane of a decoder's NV12 surface, a crop of a wider image), _img1 = the u16 depth image likewise
    // or {nullptr, 0}; for a stereo tracker (readIntrinsicParameter with two files) _img1 is the RIGHT image, 8-bit, of the same size, and the frame returns the
    // camera_id 1 observations behind the left ones (feature_tracker.cpp:259-303).  The frame size must be known (readIntrinsicParameter / setIntrinsics): a
    // device pointer carries none.  Neither image is ever written.
    FeatureFrame trackImage(double _cur_time, const gf_frame_ref& _img, const gf_frame_ref& _img1 = gf_frame_ref{nullptr, 0}, int pixel_format = GF_PIX_MONO8) {
        if (!row || !col) throw std::runtime_error("trackImage: the frame size is not known yet (readIntrinsicParameter / setIntrinsics)");
        if (!h_) { pixel_format_ = pixel_format; create(col, row); }
        if (pixel_format != pixel_format_) throw std::runtime_error("trackImage: the image's pixel format differs from the first frame's");
        std::vector<gf_feature_obs> out((size_t)((MAX_CNT + 3) & ~3) * (stereo_cam ? 2 : 1));   // both eyes
        int n = 0;
        const int seq = 0;
        check(gf_tracker_track_some_device_refs(h_, 1, &seq, &_cur_time, &_img, _img1.data ? &_img1 : nullptr, out.data(), (int)out.size(), &n));
        FeatureFrame featureFrame;
        for (int i = 0; i < n; i++) {
            Obs8 o;
            for (int k = 0; k < 8; k++) o[k] = out[i].v[k];
            featureFrame[out[i].id].emplace_back(out[i].camera_id, o);
        }
        refresh();
        return featureFrame;
    }
#ifdef GF_WITH_OPENCV
    // rgb_order: the channel order of a CV_8UC3 / CV_8UC4 image -- false: OpenCV's own B, G, R(, A) (bgr8 / bgra8), true: R, G, B(, A) (rgb8 / rgba8, what a RealSense
    // colour topic carries and cv_bridge::toCvShare hands on unconverted).  A cv::Mat does not record it, so the caller states it.
    static GrayImage viewOf(const cv::Mat& m, bool rgb_order = false) {
        if (m.depth() != CV_8U || (m.channels() != 1 && m.channels() != 3 && m.channels() != 4)) throw std::runtime_error("trackImage: the image must be CV_8UC1, CV_8UC3 or CV_8UC4");
        GrayImage g{m.ptr<uint8_t>(), m.rows, m.cols, (int)m.step};
        g.pixel_format = m.channels() == 1 ? GF_PIX_MONO8 : m.channels() == 3 ? (rgb_order ? GF_PIX_RGB8 : GF_PIX_BGR8) : (rgb_order ? GF_PIX_RGBA8 : GF_PIX_BGRA8);
        return g;
    }
    FeatureFrame trackImage(double _cur_time, const cv::Mat& _img, const cv::Mat& _img1 = cv::Mat(), bool rgb_order = false) {
        const GrayImage g = viewOf(_img, rgb_order);
        DepthImage d;
        if (!_img1.empty()) d = DepthImage{_img1.ptr<uint16_t>(), _img1.rows, _img1.cols, (int)(_img1.step / 2)};
        return trackImage(_cur_time, g, d);
    }
#endif
    void setPrediction(std::map<int, Vec3>& predictPts) {  // feature_tracker.cpp:1006-1027
        std::vector<int> pid; std::vector<double> xyz;
        for (auto& kv : predictPts) { pid.push_back(kv.first); xyz.push_back(kv.second[0]); xyz.push_back(kv.second[1]); xyz.push_back(kv.second[2]); }
        check(gf_tracker_set_prediction(h_, 0, pid.data(), xyz.data(), (int)pid.size()));
    }
    void removeOutliers(std::set<int>& removePtsIds) {  // feature_tracker.cpp:1029-1045
        std::vector<int> v(removePtsIds.begin(), removePtsIds.end());
        check(gf_tracker_remove_outliers(h_, 0, v.data(), (int)v.size()));
        refresh();
    }

  private:
    gf_tracker* h_ = nullptr;
    double fx_ = 1, fy_ = 1, cx_ = 0, cy_ = 0, k1_ = 0, k2_ = 0, p1_ = 0, p2_ = 0;
    gf_camera_model_ex camera_{};   // readIntrinsicParameter's model; GF_CAMERA_PINHOLE (also by default): the eight numbers above
    bool equalize_ = false, show_track_ = false;
    int pixel_format_ = GF_PIX_MONO8;
    std::vector<uint8_t> roi_;   // a region of interest set before the handle exists (tight rows)
    std::vector<gf_box> boxes_;  // exclusion boxes set before the handle exists
    gf_depth_reg depth_reg_{}; bool has_depth_reg_ = false;   // setDepthRegistration, kept for a handle that does not exist yet
    gf_reject_f_cfg reject_f_{};                              // setRejectWithF, likewise
    gf_stereo_cfg stereo_{};                                  // readIntrinsicParameter's second file, likewise
    gf_stereo_depth_cfg stereo_depth_{};                      // setStereoDepth, likewise
    static void check(int rc) { if (rc != GF_OK) throw std::runtime_error(std::string("groundfusion_hip: ") + gf_last_error()); }
    void create(int w, int h) {
        gf_tracker_cfg c{};
        c.width = col ? col : w; c.height = row ? row : h; c.batch = 1; c.max_cnt = MAX_CNT; c.min_dist = MIN_DIST; c.flow_back = FLOW_BACK; c.depth_cam = depth_cam ? 1 : 0;
        c.fx = fx_; c.fy = fy_; c.cx = cx_; c.cy = cy_; c.k1 = k1_; c.k2 = k2_; c.p1 = p1_; c.p2 = p2_;
        c.equalize = equalize_ ? 1 : 0;
        c.pixel_format = pixel_format_;
        row = c.height; col = c.width;
        check(gf_tracker_create(&c, &h_));
        if (camera_.model != GF_CAMERA_PINHOLE) check(gf_tracker_set_seq_camera_ex(h_, 0, &camera_));
        if (!roi_.empty()) { check(gf_tracker_set_roi(h_, 0, roi_.data(), col)); roi_.clear(); }
        if (!boxes_.empty()) { const std::vector<gf_box> b = std::move(boxes_); boxes_.clear(); setBoxes(b.data(), (int)b.size()); }
        if (show_track_) setShowTrack(true);
        if (has_depth_reg_) check(gf_tracker_set_seq_depth_reg(h_, 0, &depth_reg_));
        if (reject_f_.enable) check(gf_tracker_set_seq_reject_f(h_, 0, &reject_f_));
        if (stereo_.enable) check(gf_tracker_set_seq_stereo(h_, 0, &stereo_));
        if (stereo_depth_.enable) check(gf_tracker_set_seq_stereo_depth(h_, 0, &stereo_depth_));
    }
    void refresh() {
        const int cap = (MAX_CNT + 3) & ~3;
        ids.assign(cap, 0); track_cnt.assign(cap, 0);
        std::vector<float> p(2 * cap);
        int n = 0;
        check(gf_tracker_get_state(h_, 0, ids.data(), track_cnt.data(), p.data(), cap, &n));
        ids.resize(n); track_cnt.resize(n); prev_pts.resize(n);
        for (int i = 0; i < n; i++) prev_pts[i] = {p[2 * i], p[2 * i + 1]};
        for (int id : ids) n_id = id + 1 > n_id ? id + 1 : n_id;
    }
};

}  // namespace gf
