// Stand-in for the third-party image header that the reference's hw8 scene.cpp includes.  That file uses one function of it, in
// Scene's destructor; ref_hw8_scene.cpp defines it.  The decoders the reference's loader takes from the real header are not needed here.
#pragma once
extern "C" void stbi_image_free(void *);
