// Stand-in for <opencv2/core/core.hpp>, written for oracle/Makefile.ref: the least the reference's vendored DBoW2 needs from OpenCV
// to compile where there is no OpenCV.  TEST INFRASTRUCTURE ONLY; nothing here comes from OpenCV's sources.
//
//   cv::Mat          a rows x cols byte buffer with create / zeros / clone / release / ptr<T>().  Copies are deep (OpenCV shares
//                    the buffer between copies); DBoW2's transform and text loader never write through a copy, so they cannot tell.
//   cv::FileStorage  the members TemplatedVocabulary's YAML save / load name.  They do nothing: the harness never calls them.
//   cv::FileNode
//
// Mat::create ZERO-FILLS.  Real OpenCV leaves the memory uninitialised, so NO GOLDEN MAY DEPEND ON THAT ZERO FILL: a value the
// reference reads without having written it (the descriptor of the phantom node that a trailing newline in the vocabulary text
// makes, FORB::fromString on an empty string) must stay out of tests/golden.  tools/gen_bow_golden.py keeps it out.
//
// The real header pulls these in transitively, and the reference's sources rely on that:
#ifndef ORACLE_CVSTUB_OPENCV2_CORE_CORE_HPP
#define ORACLE_CVSTUB_OPENCV2_CORE_CORE_HPP
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>

#define CV_8U 0
#define CV_32F 5

namespace cv {

class Mat {
public:
    int rows, cols;

    Mat() : rows(0), cols(0), elem_(1) {}

    void create(int r, int c, int type) {
        rows = r;
        cols = c;
        elem_ = type == CV_32F ? 4 : 1;
        buf_.assign((size_t)r * (size_t)c * elem_, 0);
    }
    static Mat zeros(int r, int c, int type) {
        Mat m;
        m.create(r, c, type);
        return m;
    }
    Mat clone() const { return *this; }
    void release() {
        rows = cols = 0;
        buf_.clear();
    }
    bool empty() const { return buf_.empty(); }

    template <class T> T* ptr(int row = 0) { return reinterpret_cast<T*>(buf_.data() + (size_t)row * cols * elem_); }
    template <class T> const T* ptr(int row = 0) const { return reinterpret_cast<const T*>(buf_.data() + (size_t)row * cols * elem_); }

private:
    size_t elem_;
    std::vector<unsigned char> buf_;   // the heap's alignment covers the int32 reads of FORB::distance
};

class FileNode {
public:
    FileNode operator[](const char*) const { return FileNode(); }
    FileNode operator[](const std::string&) const { return FileNode(); }
    FileNode operator[](int) const { return FileNode(); }
    size_t size() const { return 0; }
    operator int() const { return 0; }
    operator double() const { return 0.0; }
    operator std::string() const { return std::string(); }
};

class FileStorage {
public:
    enum { READ = 0, WRITE = 1 };
    FileStorage(const std::string&, int) {}
    bool isOpened() const { return false; }
    FileNode operator[](const std::string&) const { return FileNode(); }
};

template <class T> inline FileStorage& operator<<(FileStorage& fs, const T&) { return fs; }

}  // namespace cv

#endif
