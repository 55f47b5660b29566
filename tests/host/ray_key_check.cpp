// Host harness of the binning key (tests/test_ray_order.py): tn_ray_key.h -- the function k_ray_keys runs per lane -- compiled
// with g++ -ffp-contract=off.  Reads <in>: float32 lo[3], hi[3], then R x (origin[3], direction[3]); writes <out>: R uint32 keys.
#include <cstdio>
#include <vector>

#include "tn_ray_key.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    float box[6];
    if (std::fread(box, sizeof(float), 6, f) != 6) return 4;
    std::vector<float> rays;
    float r[6];
    while (std::fread(r, sizeof(float), 6, f) == 6) rays.insert(rays.end(), r, r + 6);
    std::fclose(f);
    const tn::RayKeyBox b = tn::ray_key_box(box, box + 3);
    std::vector<uint32_t> keys(rays.size() / 6);
    for (size_t i = 0; i < keys.size(); ++i) {
        const float *q = rays.data() + 6 * i;
        keys[i] = tn::ray_key(q[0], q[1], q[2], q[3], q[4], q[5], b);
    }
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 5;
    std::fwrite(keys.data(), sizeof(uint32_t), keys.size(), o);
    std::fclose(o);
    return 0;
}
