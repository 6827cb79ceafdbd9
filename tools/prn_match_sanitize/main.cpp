// Stand-alone driver of mpn_prn_match_host (csrc/prn_assign.hip) for a host sanitizer run: reads one dumped case, calls the function
// on heap arrays of exactly the sizes the ABI states (so AddressSanitizer sees any access past them, and any overrun of the
// function's fixed stack tables), and writes out_kp / tie_flags for the driver script to compare.
//   case file: int32 header {nimg, nb, npeaks, cap, H, W}, then box_start[nimg+1] i32, boxes[nb*4] f64, joint_off[nimg*18] i32,
//   peaks[npeaks*2] f64, cand_n[nb*17] i32, cand_id[nb*17*cap] i32, cand_score[nb*17*cap] f32, argmax[nb*17] i32.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mpn.h"

template <typename T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); }
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s case.bin result.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int32_t> h = rd<int32_t>(f, 6);
    const size_t nimg = h[0], nb = h[1], np = h[2], cap = h[3];
    const std::vector<int32_t> box_start = rd<int32_t>(f, nimg + 1);
    const std::vector<double> boxes = rd<double>(f, nb * 4);
    const std::vector<int32_t> joint_off = rd<int32_t>(f, nimg * 18);
    const std::vector<double> peaks = rd<double>(f, np * 2);
    const std::vector<int32_t> cand_n = rd<int32_t>(f, nb * 17);
    const std::vector<int32_t> cand_id = rd<int32_t>(f, nb * 17 * cap);
    const std::vector<float> cand_score = rd<float>(f, nb * 17 * cap);
    const std::vector<int32_t> argmax = rd<int32_t>(f, nb * 17);
    fclose(f);
    std::vector<double> out_kp(nb * 51, 0.0);
    std::vector<uint8_t> flags(nimg * 17, 0);
    const int st = mpn_prn_match_host((int)nimg, box_start.data(), boxes.data(), joint_off.data(), peaks.data(), cand_n.data(), cand_id.data(),
                                      cand_score.data(), (int)cap, argmax.data(), h[4], h[5], out_kp.data(), flags.data());
    if (st != 0) { fprintf(stderr, "mpn_prn_match_host returned %d\n", st); return 3; }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    fwrite(out_kp.data(), sizeof(double), out_kp.size(), o);
    fwrite(flags.data(), 1, flags.size(), o);
    fclose(o);
    return 0;
}
