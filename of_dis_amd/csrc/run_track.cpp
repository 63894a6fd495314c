// run_track.cpp -- the run_OF_TRACK_{INT,RGB} command lines: points followed along a list of video frames.
//
//   run_OF_TRACK_INT <points.txt> <tracks.txt> <oppoint 1-4> <fb 0|1> img0 img1 ... img(T-1)
//
// points.txt: one point per line, `x y [start]` in pixels of img0's grid (start: the frame at which the point enters,
// default 0); blank lines and lines starting with '#' are skipped.  tracks.txt: one line `point frame x y status` per
// point and frame, frame-major, the coordinates as %.9g (a float32 round trip); status 0 tracked, 1 tracked past a failed
// forward-backward check (fb = 1), 2 left the frame, 3 not started.  The numbers are those of
// ofdis_run_sequence_track_u8_host on the whole list: one context, every image decoded once, every frame's pyramid
// built once.  SELECTCHANNEL (1 gray, 3 BGR) is compile-time, as in run_dense.cpp; all images must have one size.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ofdis.h"

#ifndef SELECTCHANNEL
#define SELECTCHANNEL 1
#endif
#define NOCHANNELS (SELECTCHANNEL == 3 ? 3 : 1)

// a whole decimal number in [lo, hi], or -1
static int parse_int(const char *s, int lo, int hi) {
  char *end = nullptr;
  const long v = std::strtol(s, &end, 10);
  if (end == s || *end != '\0' || v < lo || v > hi) return -1;
  return (int)v;
}

static bool read_error(const char *path, int rc) {
  std::fprintf(stderr, "cannot read %s (PNG, Netpbm or BMP expected): %s\n", path, ofdis_status_string(rc));
  return false;
}

// Every image's size (a PNG's from its header alone), before anything is computed: all must equal the first's.
static bool check_sizes(int n, char **paths, int &w, int &h) {
  for (int i = 0; i < n; ++i) {
    int iw = 0, ih = 0;
    const int rc = ofdis_read_image(paths[i], nullptr, &iw, &ih, NOCHANNELS, 0);
    if (rc != OFDIS_OK) return read_error(paths[i], rc);
    if (i == 0) {
      w = iw;
      h = ih;
    } else if (iw != w || ih != h) {
      std::fprintf(stderr, "image sizes differ: %s is %dx%d, %s is %dx%d\n", paths[i], iw, ih, paths[0], w, h);
      return false;
    }
  }
  return true;
}

// `x y [start]` per line
static bool read_points(const char *path, std::vector<float> &pts, std::vector<int32_t> &start) {
  std::FILE *f = std::fopen(path, "r");
  if (!f) {
    std::fprintf(stderr, "cannot read points file %s\n", path);
    return false;
  }
  char line[512];
  int lineno = 0;
  bool ok = true;
  while (ok && std::fgets(line, sizeof(line), f)) {
    ++lineno;
    const char *s = line + std::strspn(line, " \t\r\n");
    if (*s == '\0' || *s == '#') continue;
    float x = 0.f, y = 0.f;
    int st = 0, used = 0;
    const int got = std::sscanf(s, "%f %f%n %d%n", &x, &y, &used, &st, &used);
    if (got < 2 || s[used + std::strspn(s + used, " \t\r\n")] != '\0') {
      std::fprintf(stderr, "%s:%d: expected `x y [start]`\n", path, lineno);
      ok = false;
    } else {
      pts.push_back(x);
      pts.push_back(y);
      start.push_back(got >= 3 ? st : 0);
    }
  }
  std::fclose(f);
  if (ok && start.empty()) {
    std::fprintf(stderr, "cannot read points file %s: no points\n", path);
    ok = false;
  }
  return ok;
}

int main(int argc, char **argv) {
  const int op = argc >= 4 ? parse_int(argv[3], 1, 4) : -1;
  const int fb = argc >= 5 ? parse_int(argv[4], 0, 1) : -1;
  const int nframes = argc - 5;
  if (argc < 7 || op < 0 || fb < 0) {
    std::fprintf(stderr,
                 "usage: %s <points.txt> <tracks.txt> <oppoint 1-4> <fb 0|1> img0 img1 ... (two images or more)\n"
                 "       points.txt: `x y [start]` per line -> tracks.txt: `point frame x y status` per line\n",
                 argv[0]);
    return 1;
  }
  int w = 0, h = 0;
  if (!check_sizes(nframes, argv + 5, w, h)) return 1;
  std::vector<float> pts;
  std::vector<int32_t> start;
  if (!read_points(argv[1], pts, start)) return 1;
  const int npts = (int)start.size();
  const size_t in_frame = (size_t)w * h * NOCHANNELS;
  std::vector<uint8_t> frames(in_frame * nframes);
  for (int i = 0; i < nframes; ++i) {  // the one decode of each image
    int iw = 0, ih = 0;
    const int rc = ofdis_read_image(argv[5 + i], frames.data() + i * in_frame, &iw, &ih, NOCHANNELS, in_frame);
    if (rc != OFDIS_OK) return read_error(argv[5 + i], rc), 1;
    if (iw != w || ih != h) {  // (the file changed since check_sizes)
      std::fprintf(stderr, "image sizes differ: %s is %dx%d, expected %dx%d\n", argv[5 + i], iw, ih, w, h);
      return 1;
    }
  }
  ofdis_params p;
  int rc = ofdis_params_oppoint(&p, op, w, 1, NOCHANNELS);
  if (rc == OFDIS_OK) rc = ofdis_params_validate(&p, -1, -1, -1);
  if (rc != OFDIS_OK) {
    std::fprintf(stderr, "invalid parameters: %s\n", ofdis_status_string(rc));
    return 1;
  }
  ofdis_context *ctx = nullptr;
  rc = ofdis_context_create(0, &ctx);
  if (rc != OFDIS_OK) {
    std::fprintf(stderr, "no usable gfx950 device: %s\n", ofdis_status_string(rc));
    return 1;
  }
  std::vector<float> tracks((size_t)nframes * npts * 2);
  std::vector<uint8_t> status((size_t)nframes * npts);
  rc = ofdis_run_sequence_track_u8_host(ctx, frames.data(), nframes, w, h, &p, pts.data(), start.data(), npts, fb, 0.01f,
                                        0.5f, 0, tracks.data(), status.data());
  ofdis_context_destroy(ctx);
  if (rc != OFDIS_OK) {
    std::fprintf(stderr, "tracking failed: %s\n", ofdis_status_string(rc));
    return 1;
  }
  std::FILE *out = std::fopen(argv[2], "w");
  if (!out) {
    std::fprintf(stderr, "cannot write %s\n", argv[2]);
    return 1;
  }
  for (int j = 0; j < nframes; ++j)
    for (int k = 0; k < npts; ++k) {
      const size_t e = (size_t)j * npts + k;
      std::fprintf(out, "%d %d %.9g %.9g %d\n", k, j, tracks[2 * e], tracks[2 * e + 1], (int)status[e]);
    }
  if (std::fclose(out) != 0) {
    std::fprintf(stderr, "cannot write %s\n", argv[2]);
    return 1;
  }
  return 0;
}
