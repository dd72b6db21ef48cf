// Stand-in for the OpenCV 2.4 headers that the reference's ORB_SLAM2/src/ORBextractor.cc and include/ORBextractor.h name, written
// for oracle/Makefile.ref (target orb_ref_harness) from the call sites in those two files.  TEST INFRASTRUCTURE ONLY; nothing here
// comes from OpenCV's sources.  oracle/cvstub/ (the DBoW2 stand-in, whose Mat copies deeply) is a different header on purpose.
//
//   cv::Mat        a VIEW onto a shared 8-bit buffer: copies, rowRange / colRange / operator()(Rect) share it; clone() does not.
//                  create() keeps the buffer when size and type already match (ComputePyramid writes through views that way), and
//                  `m = Mat::zeros(..)` fills in place under the same condition (computeDescriptors writes its rows that way).
//   cv::KeyPoint, Point_, Size, Rect, InputArray, OutputArray: the members ORBextractor.cc uses.
//
// The SIX OpenCV PRIMITIVES are not OpenCV here.  Each hands its arguments to the function that oracle/orb_oracle.cc exports, so the
// harness pins everything the reference wrote itself and nothing about these:
//   FAST -> orb_oracle_fast      resize -> orb_oracle_resize      GaussianBlur -> orb_oracle_blur
//   copyMakeBorder -> orb_oracle_fill_border      fastAtan2 -> orb_oracle_fast_atan2      cvRound / cvFloor / cvCeil -> orb_oracle_round / _floor / _ceil
// Arguments other than the ones ORBextractor.cc passes abort.
#ifndef ORACLE_CVSTUB_ORB_OPENCV2_CORE_CORE_HPP
#define ORACLE_CVSTUB_ORB_OPENCV2_CORE_CORE_HPP
#include <stdint.h>
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <list>
#include <memory>
#include <utility>
#include <vector>

typedef unsigned char uchar;

#define CV_8U 0
#define CV_8UC1 0
#define CV_PI 3.1415926535897932384626433832795

extern "C" {
int orb_oracle_fast(const uint8_t* img, int cols, int rows, int step, int threshold, int32_t* xys, int cap);
void orb_oracle_resize(const uint8_t* src, int sw, int sh, int sstride, uint8_t* dst, int dw, int dh, int dstride);
void orb_oracle_blur(const uint8_t* src, int w, int h, int sstride, uint8_t* dst, int dstride);
void orb_oracle_fill_border(uint8_t* roi, int w, int h, int stride);
float orb_oracle_fast_atan2(float y, float x);
int orb_oracle_round(double v);
int orb_oracle_floor(double v);
int orb_oracle_ceil(double v);
}

inline int cvRound(double v) { return orb_oracle_round(v); }
inline int cvFloor(double v) { return orb_oracle_floor(v); }
inline int cvCeil(double v) { return orb_oracle_ceil(v); }

namespace cv {

inline void stub_abort(const char* what) {
    std::fprintf(stderr, "cvstub_orb: %s\n", what);
    std::abort();
}

template <class T> struct Point_ {
    T x, y;
    Point_() : x(0), y(0) {}
    Point_(T x_, T y_) : x(x_), y(y_) {}
};
typedef Point_<int> Point2i;
typedef Point_<int> Point;
typedef Point_<float> Point2f;
template <class T> inline Point_<T>& operator*=(Point_<T>& a, float b) {
    a.x = (T)(a.x * b);
    a.y = (T)(a.y * b);
    return a;
}

struct Size {
    int width, height;
    Size() : width(0), height(0) {}
    Size(int w, int h) : width(w), height(h) {}
};

struct Rect {
    int x, y, width, height;
    Rect() : x(0), y(0), width(0), height(0) {}
    Rect(int x_, int y_, int w, int h) : x(x_), y(y_), width(w), height(h) {}
};

struct KeyPoint {
    Point2f pt;
    float size, angle, response;
    int octave, class_id;
    KeyPoint() : size(0), angle(-1), response(0), octave(0), class_id(-1) {}
    KeyPoint(float x, float y, float size_, float angle_ = -1, float response_ = 0, int octave_ = 0, int class_id_ = -1)
        : pt(x, y), size(size_), angle(angle_), response(response_), octave(octave_), class_id(class_id_) {}
};

struct MatExpr {   // what Mat::zeros returns: assigned to a Mat of the same size it fills that Mat's own memory
    int rows, cols, type;
};

class Mat {
public:
    int rows, cols;
    size_t step;
    uchar* data;

    Mat() : rows(0), cols(0), step(0), data(0), x0_(0), y0_(0) {}
    Mat(int r, int c, int type) : rows(0), cols(0), step(0), data(0), x0_(0), y0_(0) { create(r, c, type); }
    Mat(Size sz, int type) : rows(0), cols(0), step(0), data(0), x0_(0), y0_(0) { create(sz.height, sz.width, type); }
    Mat(const MatExpr& e) : rows(0), cols(0), step(0), data(0), x0_(0), y0_(0) { *this = e; }

    void create(int r, int c, int type) {
        if (type != CV_8UC1) stub_abort("Mat::create: only CV_8UC1");
        if (data && rows == r && cols == c) return;
        buf_ = std::make_shared<Whole>();
        buf_->rows = r;
        buf_->cols = c;
        buf_->bytes.assign((size_t)r * c + 1, 0);
        rows = r; cols = c; step = (size_t)c; data = buf_->bytes.data(); x0_ = y0_ = 0;
    }
    void create(Size sz, int type) { create(sz.height, sz.width, type); }
    static MatExpr zeros(int r, int c, int type) {
        MatExpr e = {r, c, type};
        return e;
    }
    Mat& operator=(const MatExpr& e) {
        create(e.rows, e.cols, e.type);
        for (int r = 0; r < rows; ++r) std::memset(data + (size_t)r * step, 0, (size_t)cols);
        return *this;
    }
    void release() {
        buf_.reset();
        rows = cols = 0; step = 0; data = 0; x0_ = y0_ = 0;
    }
    Mat clone() const {
        Mat m;
        if (!data) return m;
        m.create(rows, cols, CV_8UC1);
        for (int r = 0; r < rows; ++r) std::memcpy(m.data + (size_t)r * m.step, data + (size_t)r * step, (size_t)cols);
        return m;
    }
    bool empty() const { return data == 0 || rows == 0 || cols == 0; }
    int type() const { return CV_8UC1; }
    size_t step1() const { return step; }

    template <class T> T& at(int r, int c) { return *reinterpret_cast<T*>(data + (ptrdiff_t)r * (ptrdiff_t)step + c); }
    template <class T> const T& at(int r, int c) const { return *reinterpret_cast<const T*>(data + (ptrdiff_t)r * (ptrdiff_t)step + c); }
    uchar* ptr(int r = 0) { return data + (size_t)r * step; }
    const uchar* ptr(int r = 0) const { return data + (size_t)r * step; }
    template <class T> T* ptr(int r = 0) { return reinterpret_cast<T*>(data + (size_t)r * step); }
    template <class T> const T* ptr(int r = 0) const { return reinterpret_cast<const T*>(data + (size_t)r * step); }

    Mat operator()(const Rect& r) const {
        if (r.x < 0 || r.y < 0 || r.width < 0 || r.height < 0 || r.x + r.width > cols || r.y + r.height > rows) stub_abort("Mat: view out of range");
        Mat m(*this);
        m.rows = r.height; m.cols = r.width;
        m.data = data + (size_t)r.y * step + r.x;
        m.x0_ = x0_ + r.x; m.y0_ = y0_ + r.y;
        return m;
    }
    // ORBextractor.cc:827 hands floats to these: the conversion is the language's (truncation)
    Mat rowRange(int a, int b) const { return (*this)(Rect(0, a, cols, b - a)); }
    Mat colRange(int a, int b) const { return (*this)(Rect(a, 0, b - a, rows)); }

    // the buffer this view looks into, and where the view starts in it
    void locateROI(Size& whole, Point& ofs) const {
        whole = buf_ ? Size(buf_->cols, buf_->rows) : Size();
        ofs = Point(x0_, y0_);
    }

private:
    struct Whole {
        int rows, cols;
        std::vector<uchar> bytes;
    };
    std::shared_ptr<Whole> buf_;
    int x0_, y0_;
};

class _InputArray {
public:
    _InputArray() : m_(0) {}
    _InputArray(const Mat& m) : m_(const_cast<Mat*>(&m)) {}
    bool empty() const { return !m_ || m_->empty(); }
    Mat getMat() const { return m_ ? *m_ : Mat(); }

protected:
    Mat* m_;
};
class _OutputArray : public _InputArray {
public:
    _OutputArray(Mat& m) : _InputArray(m) {}
    void create(int r, int c, int type) const { m_->create(r, c, type); }
    void create(Size sz, int type) const { m_->create(sz, type); }
    void release() const { m_->release(); }
};
typedef const _InputArray& InputArray;
typedef const _OutputArray& OutputArray;

enum { INTER_NEAREST = 0, INTER_LINEAR = 1 };
enum { BORDER_CONSTANT = 0, BORDER_REPLICATE = 1, BORDER_REFLECT = 2, BORDER_WRAP = 3, BORDER_REFLECT_101 = 4, BORDER_REFLECT101 = 4, BORDER_DEFAULT = 4,
       BORDER_ISOLATED = 16 };

inline float fastAtan2(float y, float x) { return orb_oracle_fast_atan2(y, x); }

// cv::FAST(image, keypoints, threshold, nonmaxSuppression = true): positions relative to the view, size 7, angle -1, response = score
inline void FAST(InputArray image, std::vector<KeyPoint>& keypoints, int threshold, bool nonmaxSuppression = true) {
    if (!nonmaxSuppression) stub_abort("FAST: only with non-maximum suppression");
    Mat m = image.getMat();
    keypoints.clear();
    if (m.empty()) return;
    std::vector<int32_t> xys((size_t)m.rows * m.cols * 3 + 3);
    int n = orb_oracle_fast(m.data, m.cols, m.rows, (int)m.step, threshold, xys.data(), m.rows * m.cols);
    for (int i = 0; i < n; ++i) keypoints.push_back(KeyPoint((float)xys[3 * i], (float)xys[3 * i + 1], 7.f, -1.f, (float)xys[3 * i + 2]));
}

inline void resize(InputArray src, OutputArray dst, Size dsize, double fx = 0, double fy = 0, int interpolation = INTER_LINEAR) {
    if (interpolation != INTER_LINEAR || fx != 0 || fy != 0 || dsize.width <= 0 || dsize.height <= 0) stub_abort("resize: only (dsize, 0, 0, INTER_LINEAR)");
    Mat s = src.getMat();
    dst.create(dsize, s.type());
    Mat d = dst.getMat();
    orb_oracle_resize(s.data, s.cols, s.rows, (int)s.step, d.data, d.cols, d.rows, (int)d.step);
}

inline void GaussianBlur(InputArray src, OutputArray dst, Size ksize, double sigmaX, double sigmaY = 0, int borderType = BORDER_DEFAULT) {
    if (ksize.width != 7 || ksize.height != 7 || sigmaX != 2 || sigmaY != 2 || borderType != BORDER_REFLECT_101) stub_abort("GaussianBlur: only (7x7, 2, 2, REFLECT_101)");
    Mat s = src.getMat().clone();   // the call site blurs in place
    dst.create(s.rows, s.cols, s.type());
    Mat d = dst.getMat();
    orb_oracle_blur(s.data, s.cols, s.rows, (int)s.step, d.data, (int)d.step);
}

inline void copyMakeBorder(InputArray src, OutputArray dst, int top, int bottom, int left, int right, int borderType) {
    if (top != 19 || bottom != 19 || left != 19 || right != 19 || (borderType & ~BORDER_ISOLATED) != BORDER_REFLECT_101)
        stub_abort("copyMakeBorder: only (19, 19, 19, 19, BORDER_REFLECT_101 [+ BORDER_ISOLATED])");
    Mat s = src.getMat();
    dst.create(s.rows + top + bottom, s.cols + left + right, s.type());   // keeps dst's memory when it already has that size
    Mat d = dst.getMat();
    uchar* roi = d.data + (size_t)top * d.step + left;
    for (int r = 0; r < s.rows; ++r)
        if (roi + (size_t)r * d.step != s.data + (size_t)r * s.step) std::memmove(roi + (size_t)r * d.step, s.data + (size_t)r * s.step, (size_t)s.cols);
    orb_oracle_fill_border(roi, s.cols, s.rows, (int)d.step);
}

// named by ComputeKeyPointsOld alone, which nothing calls
struct KeyPointsFilter {
    static void retainBest(std::vector<KeyPoint>&, int) { stub_abort("KeyPointsFilter::retainBest is not provided"); }
};

}  // namespace cv
#endif
