/*
 * oracle/ref/win_stub/winbase.h -- TEST INFRASTRUCTURE ONLY.
 *
 * Deliberately empty, like windows.h beside it: the reference's raytracer.cpp
 * includes "winbase.h" and uses nothing from it.
 */
