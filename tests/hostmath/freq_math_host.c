/* Host build of csrc/freq_math.h for tests/test_nerf_background_host.py, a stand-alone program:
 *     freq_math_host <degree> <n>  < n directions [n, 3] fp32  > their encodings [n, 3 + 6 degree] fp32 */
#include <stdio.h>
#include <stdlib.h>

#include "../../dreamwaltz-g_amd/csrc/freq_math.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const long degree = strtol(argv[1], NULL, 10), n = strtol(argv[2], NULL, 10);
    if (degree < 1 || degree > (long)DWG_FREQ_MAX_DEGREE || n < 0) return 2;
    const uint32_t k = freq_output_dim((uint32_t)degree);
    float x[3], out[3 + 6 * DWG_FREQ_MAX_DEGREE];
    for (long i = 0; i < n; ++i) {
        if (fread(x, sizeof(float), 3, stdin) != 3) return 3;
        freq_encode(x, (uint32_t)degree, out);
        if (fwrite(out, sizeof(float), k, stdout) != k) return 4;
    }
    return 0;
}
