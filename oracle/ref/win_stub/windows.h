/*
 * oracle/ref/win_stub/windows.h -- TEST INFRASTRUCTURE ONLY.
 *
 * Deliberately empty.  The reference's raytracer.cpp includes "windows.h" but
 * uses nothing from it (Engine_Raytrace / Engine_Render are plain C++ and
 * libm), so this directory is put first on the include path and the file is
 * compiled where it lies, unmodified (oracle/Makefile, target ref).
 */
