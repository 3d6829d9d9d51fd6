// Stream sources / sinks (include/rebvio/io/stream_io.hpp). PNG decoding = chunk walk + zlib inflate + the five PNG
// scanline filters; nothing else of libpng is needed for camera frames.
#include "rebvio/io/stream_io.hpp"

#include <zlib.h>

#include "../csrc/pixel_format.hpp"

#include <algorithm>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>

namespace rebvio {
namespace io {

namespace {
[[noreturn]] void bad(const std::string& what) { throw std::runtime_error(what); }

std::vector<unsigned char> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) bad("cannot open " + path);
  const std::streamsize n = f.tellg();
  f.seekg(0);
  std::vector<unsigned char> b((size_t)n);
  if (n > 0 && !f.read(reinterpret_cast<char*>(b.data()), n)) bad("cannot read " + path);
  return b;
}
inline uint32_t be32(const unsigned char* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
inline int paeth(int a, int b, int c) {
  const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
std::string trim(const std::string& s) {
  size_t a = 0, b = s.size();
  while (a < b && (s[a] == ' ' || s[a] == '\t' || s[a] == '\r' || s[a] == '\n')) ++a;
  while (b > a && (s[b - 1] == ' ' || s[b - 1] == '\t' || s[b - 1] == '\r' || s[b - 1] == '\n')) --b;
  return s.substr(a, b - a);
}
std::vector<std::string> csv_fields(const std::string& line) {
  std::vector<std::string> out;
  std::stringstream ss(line);
  std::string f;
  while (std::getline(ss, f, ',')) out.push_back(trim(f));
  return out;
}
}  // namespace

namespace {
// Decodes a PNG file: W, H and the colour type are set once the header is read, then begin(W, H) is called, then
// row(y, bytes, bytes_per_pixel) for every image row with its unfiltered bytes.
template <class BeginFn, class RowFn>
void decodePng(const std::string& path, uint32_t& W, uint32_t& H, int& ctype, BeginFn begin, RowFn row) {
  const std::vector<unsigned char> file = slurp(path);
  static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
  if (file.size() < 8 + 25 || std::memcmp(file.data(), sig, 8) != 0) bad(path + ": not a PNG file");
  W = 0, H = 0;
  ctype = 0;
  int depth = 0, interlace = 0;
  std::vector<unsigned char> idat;
  size_t pos = 8;
  bool end = false;
  while (!end && pos + 12 <= file.size()) {
    const uint32_t len = be32(&file[pos]);
    const char* type = reinterpret_cast<const char*>(&file[pos + 4]);
    if (pos + 12 + (size_t)len > file.size()) bad(path + ": truncated chunk");
    const unsigned char* data = &file[pos + 8];
    if (!std::memcmp(type, "IHDR", 4)) {
      if (len < 13) bad(path + ": bad IHDR");
      W = be32(data);
      H = be32(data + 4);
      depth = data[8];
      ctype = data[9];
      interlace = data[12];
    } else if (!std::memcmp(type, "IDAT", 4)) {
      idat.insert(idat.end(), data, data + len);
    } else if (!std::memcmp(type, "IEND", 4)) {
      end = true;
    }
    pos += 12 + (size_t)len;
  }
  if (W == 0 || H == 0 || W > 16384 || H > 16384) bad(path + ": bad size");
  if (interlace != 0) bad(path + ": interlaced PNG not supported");
  int channels;
  switch (ctype) {
    case 0: channels = 1; break;
    case 2: channels = 3; break;
    case 4: channels = 2; break;
    case 6: channels = 4; break;
    default: bad(path + ": palette PNG not supported");
  }
  if (!(depth == 8 || (depth == 16 && ctype == 0))) bad(path + ": unsupported bit depth");
  const size_t bpp = (size_t)channels * depth / 8, stride = (size_t)W * bpp;
  std::vector<unsigned char> raw((stride + 1) * H);
  uLongf out_len = (uLongf)raw.size();
  if (uncompress(raw.data(), &out_len, idat.data(), (uLong)idat.size()) != Z_OK || out_len != raw.size()) bad(path + ": inflate failed");
  std::vector<unsigned char> prev(stride, 0), cur(stride);
  begin(W, H);
  for (uint32_t y = 0; y < H; ++y) {
    const unsigned char ft = raw[(stride + 1) * y];
    const unsigned char* in = &raw[(stride + 1) * y + 1];
    for (size_t i = 0; i < stride; ++i) {
      const int a = i >= bpp ? cur[i - bpp] : 0, b = prev[i], c = i >= bpp ? prev[i - bpp] : 0;
      int v = in[i];
      switch (ft) {
        case 0: break;
        case 1: v += a; break;
        case 2: v += b; break;
        case 3: v += (a + b) >> 1; break;
        case 4: v += paeth(a, b, c); break;
        default: bad(path + ": bad filter type");
      }
      cur[i] = (unsigned char)v;
    }
    row(y, cur.data(), bpp);
    prev.swap(cur);
  }
}
}  // namespace

cv::Mat readPngGray(const std::string& path) {
  uint32_t W, H;
  int ctype;
  cv::Mat img;
  decodePng(path, W, H, ctype, [&](uint32_t w, uint32_t h) { img.create((int)h, (int)w, CV_8UC1); },
            [&](uint32_t y, const unsigned char* row, size_t bpp) {
              unsigned char* o = img.ptr<unsigned char>((int)y);
              for (uint32_t x = 0; x < W; ++x) {
                const unsigned char* px = &row[(size_t)x * bpp];
                if (ctype == 0 || ctype == 4)
                  o[x] = px[0];  // 16-bit grey: most significant byte
                else             // RGB(A) -> luma with the fixed-point weights of cv::cvtColor(RGB2GRAY)
                  o[x] = rh::px::grey_at<rh::px::RGB8>(px, 0);
              }
            });
  return img;
}

PngPixels readPngPixels(const std::string& path, bool opencv_order) {
  uint32_t W, H;
  int ctype;
  PngPixels out;
  decodePng(path, W, H, ctype,
            [&](uint32_t w, uint32_t h) {
              const int ch = (ctype == 2) ? 3 : (ctype == 6) ? 4 : 1;
              out.data.create((int)h, (int)w, ch == 3 ? CV_8UC3 : ch == 4 ? CV_8UC4 : CV_8UC1);
              out.format = ch == 3 ? (opencv_order ? REBVIO_HIP_PX_BGR8 : REBVIO_HIP_PX_RGB8)
                                   : ch == 4 ? (opencv_order ? REBVIO_HIP_PX_BGRA8 : REBVIO_HIP_PX_RGBA8) : REBVIO_HIP_PX_GRAY8;
            },
            [&](uint32_t y, const unsigned char* row, size_t bpp) {
              unsigned char* o = out.data.ptr<unsigned char>((int)y);
              if (ctype == 2 || ctype == 6) {
                const size_t ch = ctype == 2 ? 3 : 4;
                std::memcpy(o, row, (size_t)W * ch);
                if (opencv_order)
                  for (uint32_t x = 0; x < W; ++x) std::swap(o[(size_t)x * ch], o[(size_t)x * ch + 2]);
              } else {
                for (uint32_t x = 0; x < W; ++x) o[x] = row[(size_t)x * bpp];  // grey + alpha: grey; 16-bit grey: most significant byte
              }
            });
  return out;
}

EurocReader::EurocReader(const std::string& mav0, const std::string& cam, const std::string& imu, bool colour) : colour_(colour) {
  {
    const std::string dir = mav0 + "/" + cam;
    std::ifstream f(dir + "/data.csv");
    if (!f) bad("cannot open " + dir + "/data.csv");
    std::string line;
    while (std::getline(f, line)) {
      line = trim(line);
      if (line.empty() || line[0] == '#') continue;
      const auto fs = csv_fields(line);
      if (fs.size() < 2) continue;
      const uint64_t ns = std::stoull(fs[0]);
      frames_.push_back(FrameRef{ns / 1000ull, dir + "/data/" + fs[1], 0});
    }
    std::stable_sort(frames_.begin(), frames_.end(), [](const FrameRef& a, const FrameRef& b) { return a.ts_us < b.ts_us; });
  }
  {
    std::ifstream f(mav0 + "/" + imu + "/data.csv");
    if (f) {  // a camera-only dataset is allowed
      std::string line;
      while (std::getline(f, line)) {
        line = trim(line);
        if (line.empty() || line[0] == '#') continue;
        const auto fs = csv_fields(line);
        if (fs.size() < 7) continue;
        rebvio::types::Imu s;
        s.ts = std::stoull(fs[0]) / 1000ull;
        s.gyro = TooN::makeVector(std::stof(fs[1]), std::stof(fs[2]), std::stof(fs[3]));
        s.acc = TooN::makeVector(std::stof(fs[4]), std::stof(fs[5]), std::stof(fs[6]));
        imu_.push_back(s);
      }
      std::stable_sort(imu_.begin(), imu_.end(), [](const rebvio::types::Imu& a, const rebvio::types::Imu& b) { return a.ts < b.ts; });
    }
  }
}

RawReader::RawReader(const std::string& frames_file, int rows, int cols, uint64_t first_ts_us, uint64_t frame_dt_us,
                     const std::string& imu_file)
    : path_(frames_file), rows_(rows), cols_(cols), n_(0), t0_(first_ts_us), dt_(frame_dt_us) {
  std::ifstream f(frames_file, std::ios::binary | std::ios::ate);
  if (!f) bad("cannot open " + frames_file);
  n_ = (size_t)f.tellg() / ((size_t)rows * cols);
  if (!imu_file.empty()) {
    const std::vector<unsigned char> b = slurp(imu_file);
    for (size_t o = 0; o + 32 <= b.size(); o += 32) {
      int64_t ts;
      float g[3], a[3];
      std::memcpy(&ts, &b[o], 8);
      std::memcpy(g, &b[o + 8], 12);
      std::memcpy(a, &b[o + 20], 12);
      imu_.push_back(rebvio::types::Imu{(uint64_t)ts, TooN::makeVector(g[0], g[1], g[2]), TooN::makeVector(a[0], a[1], a[2])});
    }
  }
}

cv::Mat RawReader::frame(size_t i) {
  if (i >= n_) bad("RawReader: frame index out of range");
  cv::Mat m(rows_, cols_, CV_8UC1);
  std::ifstream f(path_, std::ios::binary);
  f.seekg((std::streamoff)(i * (size_t)rows_ * cols_));
  if (!f.read(reinterpret_cast<char*>(m.data), (std::streamsize)((size_t)rows_ * cols_))) bad("RawReader: short read");
  return m;
}

OdometryWriter::OdometryWriter(const std::string& path) : f_(std::fopen(path.c_str(), "w")) {
  if (!f_) bad("cannot create " + path);
}
OdometryWriter::~OdometryWriter() {
  if (f_) std::fclose(f_);
}
std::string OdometryWriter::format(const rebvio::types::Odometry& o) {
  char buf[256];
  std::snprintf(buf, sizeof(buf), "%llu %.6f %.6f %.6f %.6f %.6f %.6f", (unsigned long long)o.ts_us, (double)o.orientation[0],
                (double)o.orientation[1], (double)o.orientation[2], (double)o.position[0], (double)o.position[1], (double)o.position[2]);
  return buf;
}
void OdometryWriter::write(const rebvio::types::Odometry& o) {
  std::fprintf(f_, "%s\n", format(o).c_str());
  std::fflush(f_);
}

void writePointCloudPly(const std::string& path, const rebvio::types::CloudPoint* points, size_t n, uint64_t ts_us) {
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) bad("cannot create " + path);
  std::fprintf(f, "ply\nformat binary_little_endian 1.0\ncomment rebvio point cloud ts_us %llu\nelement vertex %zu\n"
               "property float x\nproperty float y\nproperty float z\nproperty float intensity\nend_header\n",
               (unsigned long long)ts_us, n);
  std::vector<unsigned char> body(n * 16);
  for (size_t i = 0; i < n; ++i) {
    const float v[4] = {points[i].xyz[0], points[i].xyz[1], points[i].xyz[2], points[i].gradient_norm};
    for (int k = 0; k < 4; ++k) {
      uint32_t w;
      std::memcpy(&w, &v[k], 4);
      for (int b = 0; b < 4; ++b) body[i * 16 + k * 4 + b] = (unsigned char)(w >> (8 * b));  // little-endian on any host
    }
  }
  const bool ok = body.empty() || std::fwrite(body.data(), 1, body.size(), f) == body.size();
  if (std::fclose(f) != 0 || !ok) bad("cannot write " + path);
}

std::vector<PlyVertex> readPointCloudPly(const std::string& path, uint64_t* ts_us) {
  std::FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) bad("cannot open " + path);
  std::vector<std::string> lines;
  std::string line;
  for (int c; (c = std::fgetc(f)) != EOF;) {
    if (c != '\n') {
      line.push_back((char)c);
      if (line.size() > 200) break;
      continue;
    }
    lines.push_back(line);
    if (line == "end_header") break;
    line.clear();
  }
  unsigned long long ts = 0, n = 0;
  const bool header_ok = lines.size() == 9 && lines[0] == "ply" && lines[1] == "format binary_little_endian 1.0" &&
                         std::sscanf(lines[2].c_str(), "comment rebvio point cloud ts_us %llu", &ts) == 1 &&
                         std::sscanf(lines[3].c_str(), "element vertex %llu", &n) == 1 && lines[4] == "property float x" &&
                         lines[5] == "property float y" && lines[6] == "property float z" && lines[7] == "property float intensity" &&
                         lines[8] == "end_header";
  if (!header_ok) {
    std::fclose(f);
    bad(path + ": not a point-cloud PLY file of writePointCloudPly");
  }
  std::vector<unsigned char> body((size_t)n * 16);
  const bool ok = (body.empty() || std::fread(body.data(), 1, body.size(), f) == body.size()) && std::fgetc(f) == EOF;
  std::fclose(f);
  if (!ok) bad(path + ": the vertex data do not match the header's count");
  std::vector<PlyVertex> out((size_t)n);
  for (size_t i = 0; i < out.size(); ++i) {
    float v[4];
    for (int k = 0; k < 4; ++k) {
      uint32_t w = 0;
      for (int b = 0; b < 4; ++b) w |= (uint32_t)body[i * 16 + k * 4 + b] << (8 * b);
      std::memcpy(&v[k], &w, 4);
    }
    out[i] = PlyVertex{v[0], v[1], v[2], v[3]};
  }
  if (ts_us) *ts_us = ts;
  return out;
}

namespace {
void put_le32(std::vector<unsigned char>& body, size_t at, uint32_t w) {
  for (int b = 0; b < 4; ++b) body[at + b] = (unsigned char)(w >> (8 * b));  // little-endian on any host
}
uint32_t get_le32(const std::vector<unsigned char>& body, size_t at) {
  uint32_t w = 0;
  for (int b = 0; b < 4; ++b) w |= (uint32_t)body[at + b] << (8 * b);
  return w;
}
}  // namespace

namespace {
// n vertices and the edges as a PLY file; kind = the word of the comment line ("polylines", "segments"); vertex(i) = the i-th
// vertex, read where it lies: nothing is copied in front of the file's body
template <class VertexOf>
void write_edges_ply(const std::string& path, const char* kind, size_t n, VertexOf vertex, const std::vector<PlyEdge>& edges, uint64_t ts_us) {
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) bad("cannot create " + path);
  std::fprintf(f, "ply\nformat binary_little_endian 1.0\ncomment rebvio %s ts_us %llu\nelement vertex %zu\n"
               "property float x\nproperty float y\nproperty float z\nproperty float intensity\nelement edge %zu\n"
               "property int vertex1\nproperty int vertex2\nend_header\n",
               kind, (unsigned long long)ts_us, n, edges.size());
  std::vector<unsigned char> body(n * 16 + edges.size() * 8);
  for (size_t i = 0; i < n; ++i) {
    const PlyVertex pv = vertex(i);
    const float v[4] = {pv.x, pv.y, pv.z, pv.intensity};
    for (int k = 0; k < 4; ++k) {
      uint32_t w;
      std::memcpy(&w, &v[k], 4);
      put_le32(body, i * 16 + (size_t)k * 4, w);
    }
  }
  for (size_t e = 0; e < edges.size(); ++e) {
    put_le32(body, n * 16 + e * 8, (uint32_t)edges[e].vertex1);
    put_le32(body, n * 16 + e * 8 + 4, (uint32_t)edges[e].vertex2);
  }
  const bool ok = body.empty() || std::fwrite(body.data(), 1, body.size(), f) == body.size();
  if (std::fclose(f) != 0 || !ok) bad("cannot write " + path);
}
std::vector<PlyVertex> read_edges_ply(const std::string& path, const char* kind, std::vector<PlyEdge>* edges, uint64_t* ts_us);
}  // namespace

void writePolylinesPly(const std::string& path, const rebvio::types::CloudPoint* points, size_t n, const rebvio::types::Polyline* lines,
                       size_t n_lines, uint64_t ts_us) {
  std::vector<PlyEdge> edges;
  for (size_t l = 0; l < n_lines; ++l) {
    const rebvio::types::Polyline& ln = lines[l];
    if (ln.first_point < 0 || ln.points < 1 || (size_t)ln.first_point >= n) continue;
    const size_t first = (size_t)ln.first_point, whole = first + (size_t)ln.points, end = std::min(whole, n);
    for (size_t k = first; k + 1 < end; ++k) edges.push_back(PlyEdge{(int)k, (int)k + 1});
    if ((ln.flags & 1) && end == whole && ln.points >= 2) edges.push_back(PlyEdge{(int)end - 1, (int)first});
  }
  write_edges_ply(path, "polylines", n,
                  [points](size_t i) { return PlyVertex{points[i].xyz[0], points[i].xyz[1], points[i].xyz[2], points[i].gradient_norm}; }, edges, ts_us);
}

std::vector<PlyVertex> readPolylinesPly(const std::string& path, std::vector<PlyEdge>* edges, uint64_t* ts_us) {
  return read_edges_ply(path, "polylines", edges, ts_us);
}

void writeSegmentsPly(const std::string& path, const rebvio::types::LineSegment* segments, size_t n, uint64_t ts_us) {
  std::vector<PlyVertex> vertices;
  std::vector<PlyEdge> edges;
  for (size_t i = 0; i < n; ++i) {
    const rebvio::types::LineSegment& s = segments[i];
    if (!(s.flags & 1)) continue;
    const int at = (int)vertices.size();
    vertices.push_back(PlyVertex{s.xyz0[0], s.xyz0[1], s.xyz0[2], s.sigma_rho0});
    vertices.push_back(PlyVertex{s.xyz1[0], s.xyz1[1], s.xyz1[2], s.sigma_rho1});
    edges.push_back(PlyEdge{at, at + 1});
  }
  write_edges_ply(path, "segments", vertices.size(), [&vertices](size_t i) { return vertices[i]; }, edges, ts_us);
}

std::vector<PlyVertex> readSegmentsPly(const std::string& path, std::vector<PlyEdge>* edges, uint64_t* ts_us) {
  return read_edges_ply(path, "segments", edges, ts_us);
}

namespace {
std::vector<PlyVertex> read_edges_ply(const std::string& path, const char* kind, std::vector<PlyEdge>* edges, uint64_t* ts_us) {
  std::FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) bad("cannot open " + path);
  std::vector<std::string> lines;
  std::string line;
  for (int c; (c = std::fgetc(f)) != EOF;) {
    if (c != '\n') {
      line.push_back((char)c);
      if (line.size() > 200) break;
      continue;
    }
    lines.push_back(line);
    if (line == "end_header" || lines.size() > 12) break;
    line.clear();
  }
  unsigned long long ts = 0, n = 0, m = 0;
  const bool header_ok = lines.size() == 12 && lines[0] == "ply" && lines[1] == "format binary_little_endian 1.0" &&
                         std::sscanf(lines[2].c_str(), (std::string("comment rebvio ") + kind + " ts_us %llu").c_str(), &ts) == 1 &&
                         std::sscanf(lines[3].c_str(), "element vertex %llu", &n) == 1 && lines[4] == "property float x" &&
                         lines[5] == "property float y" && lines[6] == "property float z" && lines[7] == "property float intensity" &&
                         std::sscanf(lines[8].c_str(), "element edge %llu", &m) == 1 && lines[9] == "property int vertex1" &&
                         lines[10] == "property int vertex2" && lines[11] == "end_header" && n <= (1ull << 31) && m <= (1ull << 31);
  if (!header_ok) {
    std::fclose(f);
    bad(path + (std::string(kind) == "polylines" ? ": not a polyline PLY file of writePolylinesPly" : ": not a segment PLY file of writeSegmentsPly"));
  }
  std::vector<unsigned char> body((size_t)n * 16 + (size_t)m * 8);
  const bool ok = (body.empty() || std::fread(body.data(), 1, body.size(), f) == body.size()) && std::fgetc(f) == EOF;
  std::fclose(f);
  if (!ok) bad(path + ": the vertex and edge data do not match the header's counts");
  std::vector<PlyVertex> out((size_t)n);
  for (size_t i = 0; i < out.size(); ++i) {
    float v[4];
    for (int k = 0; k < 4; ++k) {
      const uint32_t w = get_le32(body, i * 16 + (size_t)k * 4);
      std::memcpy(&v[k], &w, 4);
    }
    out[i] = PlyVertex{v[0], v[1], v[2], v[3]};
  }
  std::vector<PlyEdge> es((size_t)m);
  for (size_t e = 0; e < es.size(); ++e) {
    es[e] = PlyEdge{(int)get_le32(body, (size_t)n * 16 + e * 8), (int)get_le32(body, (size_t)n * 16 + e * 8 + 4)};
    if (es[e].vertex1 < 0 || es[e].vertex2 < 0 || (unsigned long long)es[e].vertex1 >= n || (unsigned long long)es[e].vertex2 >= n)
      bad(path + ": an edge names a vertex outside the file");
  }
  if (edges) *edges = std::move(es);
  if (ts_us) *ts_us = ts;
  return out;
}
}  // namespace

size_t replay(StreamSource& src, const std::function<void(rebvio::types::Image&&)>& image_cb,
              const std::function<void(rebvio::types::Imu&&)>& imu_cb, size_t first, size_t count) {
  const auto& imu = src.imu();
  size_t k = 0, delivered = 0;
  const size_t last = std::min(src.numFrames(), count == (size_t)-1 ? src.numFrames() : first + count);
  // samples older than the first played frame belong to nobody
  if (first < src.numFrames() && first > 0)
    while (k < imu.size() && imu[k].ts <= src.frameTs(first - 1)) ++k;
  for (size_t i = first; i < last; ++i) {
    const uint64_t ts = src.frameTs(i);
    for (; k < imu.size() && imu[k].ts <= ts; ++k)
      if (imu_cb) imu_cb(rebvio::types::Imu(imu[k]));
    image_cb(rebvio::types::Image{ts, src.frame(i)});
    ++delivered;
  }
  return delivered;
}

}  // namespace io
}  // namespace rebvio
