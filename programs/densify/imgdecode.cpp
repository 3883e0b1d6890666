// imgdecode -- decode one image with the densify CLI's ingest (load_image:
// JPEG / PNG / PPM -> BGR8, as cv::imread IMREAD_COLOR) and write it as a
// binary PPM (RGB) to the output path; used by the CPU ingest tests.
//   imgdecode in.jpg out.ppm
#include "scene_io.h"

#include <cstdio>
#include <exception>

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: imgdecode <image> <out.ppm>\n");
        return 2;
    }
    try {
        const dpio::Image im = dpio::load_image(argv[1]);
        dpio::write_ppm(argv[2], im.width, im.height, im.bgr);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
