// ikd_ref_driver.cpp — TEST INFRASTRUCTURE ONLY.  Runs the reference's own ikd-Tree
// (third_party/ikd-Tree/ikd_Tree.{h,cpp}, found on the include path; none of its text is here) on a
// job file and writes what it answered.  Built by `make -C oracle ref`; driven by oracle/ikd_ref.py.
//
//   ikd_ref job.bin result.bin
//
// Job file, little-endian:  u32 magic 'IKDJ', f32 delete_param, balance_param, box_length, then ops
// until the end of the file, each a u32 opcode and its payload.  A point is three f32 (x, y, z); its
// index, given as `first` + position, goes into the intensity (exact below 2^24).
//   1 build          u32 n, i32 first, n points           Build
//   2 add            u32 n, i32 first, u32 downsample_on, n points      Add_Points -> counter
//   3 set_downsample f32 box_length
//   4 sector         f32 cx, cy, cz, radius, heading      Sector_Search  -> indices
//   5 box            f32 min xyz, max xyz                 Box_Search     -> indices
//   6 radius         f32 cx, cy, cz, radius               Radius_Search  -> indices
//   7 delete_boxes   u32 nb, nb x 6 f32                   Delete_Point_Boxes -> deleted
//   8 size           -                                    -> size(), validnum() once the rebuild thread is idle, and
//                                                           how often a rebuild was handed to that thread so far
//   9 heading_table  u32 n, n x (point xyz, centre xyz)   -> n calc_heading bits, then n calc_dist bits
// Result file: per op, in order, u32 opcode, u32 word count, then that many 32-bit words.  Index lists
// are sorted ascending (the tree returns its pre-order).
//
// The tree is heap-allocated: it is about 64 MB by value and starts its rebuild thread.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <math.h>
#include <pthread.h>
#include <queue>
#include <stdio.h>
#include <time.h>
#include <unistd.h>

// The tree hands a subtree of 1500 points or more to its rebuild thread after a trylock on
// rebuild_ptr_mutex_lock, and tries that mutex nowhere else: counting those calls tells a test whether its
// case went through the thread at all.  (How many there are depends on the thread's timing.)
static uint32_t g_thread_requests = 0;
static const void* g_rebuild_lock = nullptr;
static int counted_trylock(pthread_mutex_t* m) {
    if (m == g_rebuild_lock) ++g_thread_requests;
    return pthread_mutex_trylock(m);
}

// calc_heading, calc_dist and the rebuild thread's state are private members; every standard header
// the tree uses is already included above, so the macros reach the tree's two files only.
#define private public
#define pthread_mutex_trylock(m) counted_trylock(m)
#include "ikd_Tree.cpp"
#undef pthread_mutex_trylock
#undef private

typedef pcl::PointXYZI PointType;
typedef KD_TREE<PointType> Tree;
typedef Tree::PointVector PointVector;

static FILE* g_in = nullptr;
static FILE* g_out = nullptr;

static void die(const char* what) {
    std::fprintf(stderr, "ikd_ref: %s\n", what);
    std::exit(2);
}

template <typename T>
static bool get(T* v, size_t n = 1) {
    return std::fread(v, sizeof(T), n, g_in) == n;
}

template <typename T>
static T need() {
    T v;
    if (!get(&v)) die("short job file");
    return v;
}

static void put_words(uint32_t op, const std::vector<uint32_t>& w) {
    const uint32_t head[2] = {op, (uint32_t)w.size()};
    if (std::fwrite(head, 4, 2, g_out) != 2 || (w.size() && std::fwrite(w.data(), 4, w.size(), g_out) != w.size()))
        die("cannot write the result file");
}

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

static PointVector read_points(uint32_t n, int32_t first) {
    if ((int64_t)first + n > (1 << 24)) die("index does not fit a float");
    std::vector<float> xyz((size_t)n * 3);
    if (n && !get(xyz.data(), xyz.size())) die("short job file");
    PointVector v(n);
    for (uint32_t i = 0; i < n; ++i) {
        v[i].x = xyz[3 * i];
        v[i].y = xyz[3 * i + 1];
        v[i].z = xyz[3 * i + 2];
        v[i].intensity = (float)(first + (int32_t)i);
    }
    return v;
}

static PointType read_point() {
    PointType p;
    p.x = need<float>();
    p.y = need<float>();
    p.z = need<float>();
    return p;
}

static void put_indices(uint32_t op, const PointVector& found) {
    std::vector<uint32_t> w(found.size());
    std::vector<int32_t> idx(found.size());
    for (size_t i = 0; i < found.size(); ++i) idx[i] = (int32_t)found[i].intensity;
    std::sort(idx.begin(), idx.end());
    for (size_t i = 0; i < idx.size(); ++i) w[i] = (uint32_t)idx[i];
    put_words(op, w);
}

// size() answers a stale count while the rebuild thread holds the root: wait until that thread has
// taken and finished whatever was handed to it (it keeps rebuild_ptr_mutex_lock for a whole rebuild).
static void wait_idle(Tree* tree) {
    for (int spin = 0; spin < 200000; ++spin) {
        pthread_mutex_lock(&tree->rebuild_ptr_mutex_lock);
        const bool idle = tree->Rebuild_Ptr == nullptr;
        pthread_mutex_unlock(&tree->rebuild_ptr_mutex_lock);
        if (idle) return;
        usleep(100);
    }
    die("the rebuild thread did not become idle");
}

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s job.bin result.bin\n", argv[0]);
        return 2;
    }
    g_in = std::fopen(argv[1], "rb");
    g_out = std::fopen(argv[2], "wb");
    if (!g_in || !g_out) die("cannot open the job or the result file");
    if (need<uint32_t>() != 0x4A444B49u) die("not a job file");
    const float delete_param = need<float>(), balance_param = need<float>(), box_length = need<float>();
    Tree* tree = new Tree(delete_param, balance_param, box_length);
    g_rebuild_lock = &tree->rebuild_ptr_mutex_lock;
    PointVector found;
    uint32_t op;
    while (get(&op)) {
        switch (op) {
        case 1: {
            const uint32_t n = need<uint32_t>();
            const int32_t first = need<int32_t>();
            tree->Build(read_points(n, first));
            put_words(op, {});
            break;
        }
        case 2: {
            const uint32_t n = need<uint32_t>();
            const int32_t first = need<int32_t>();
            const uint32_t downsample_on = need<uint32_t>();
            PointVector pts = read_points(n, first);
            put_words(op, {(uint32_t)tree->Add_Points(pts, downsample_on != 0)});
            break;
        }
        case 3:
            tree->set_downsample_param(need<float>());
            put_words(op, {});
            break;
        case 4: {
            const PointType c = read_point();
            const float radius = need<float>(), heading = need<float>();
            tree->Sector_Search(c, radius, heading, found);
            put_indices(op, found);
            break;
        }
        case 5: {
            BoxPointType box;
            if (!get(box.vertex_min, 3) || !get(box.vertex_max, 3)) die("short job file");
            tree->Box_Search(box, found);
            put_indices(op, found);
            break;
        }
        case 6: {
            const PointType c = read_point();
            tree->Radius_Search(c, need<float>(), found);
            put_indices(op, found);
            break;
        }
        case 7: {
            std::vector<BoxPointType> boxes(need<uint32_t>());
            for (BoxPointType& b : boxes)
                if (!get(b.vertex_min, 3) || !get(b.vertex_max, 3)) die("short job file");
            put_words(op, {(uint32_t)tree->Delete_Point_Boxes(boxes)});
            break;
        }
        case 8:
            wait_idle(tree);
            put_words(op, {(uint32_t)tree->size(), (uint32_t)tree->validnum(), g_thread_requests});
            break;
        case 9: {
            const uint32_t n = need<uint32_t>();
            std::vector<uint32_t> w((size_t)n * 2);
            for (uint32_t i = 0; i < n; ++i) {
                const PointType a = read_point(), b = read_point();
                w[i] = bits(tree->calc_heading(a, b));
                w[n + i] = bits(tree->calc_dist(a, b));
            }
            put_words(op, w);
            break;
        }
        default:
            die("unknown opcode");
        }
    }
    delete tree;
    if (std::fclose(g_out) != 0) die("cannot write the result file");
    return 0;
}
