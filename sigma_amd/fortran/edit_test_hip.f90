!==========================================================================!
! edit_test_hip: the flow of the reference's examples/fem.f90 through the   !
! batch edits of the stand-alone host layer.  A P1 triangulation of a       !
! jittered grid: the pattern from the element stream, then the stiffness    !
! and the mass matrix assembled ON THE DEVICE by add_values_at (one ordered !
! batch of 9 triples per element, the order of laplacian2d / mass2d's       !
! add_value calls) and compared, bit for bit, with the scalar host-mirror   !
! add_value loop; add_multiple_values element by element, scalar_multiply   !
! and set_values_at likewise; the same for the ELLPACK layer.  Then a CG    !
! solve of (A + M) u = M 1 with the edited matrix.                          !
!==========================================================================!
program edit_test_hip
use iso_c_binding
use sigma_hip
implicit none
    integer, parameter :: nx = 24, ny = 17
    integer, parameter :: nn = nx * ny, ne = 2 * (nx - 1) * (ny - 1)
    real(dp) :: x(2, nn), AE(3, 3), r
    integer :: ele(3, ne), n, i, j, cx, cy, a, t, k
    integer, allocatable :: ti(:), tj(:), ptr(:), node(:), deg(:)
    real(dp), allocatable :: tz(:), tm(:), u(:), b(:), ones(:)
    type(hip_csr_matrix) :: Ad, Ah, Md
    type(hip_ellpack_matrix) :: Ed, Eh
    type(hip_linear_solver), pointer :: solver
    logical :: seen(nn)
    integer :: fails

    fails = 0
    call hip_check(sgm_init(0_c_int))
    ! jittered coordinates: dyadic ones would hide the order of the additions
    k = 12345
    do n = 1, nn
        do i = 1, 2
            k = mod(k * 1103 + 12347, 65536)
            r = (real(k, dp) / 65536.0_dp - 0.5_dp) * 0.2_dp
            if (i == 1) x(i, n) = real(mod(n - 1, nx), dp) + r
            if (i == 2) x(i, n) = real((n - 1) / nx, dp) + r
        enddo
    enddo
    n = 0
    do cy = 0, ny - 2
        do cx = 0, nx - 2
            a = cy * nx + cx + 1
            ele(:, n + 1) = [a, a + 1, a + nx + 1]
            ele(:, n + 2) = [a, a + nx + 1, a + nx]
            n = n + 2
        enddo
    enddo

    ! the triple streams of laplacian2d / mass2d (fem.f90:28-49, 68-87)
    allocate(ti(9 * ne), tj(9 * ne), tz(9 * ne), tm(9 * ne))
    t = 0
    do n = 1, ne
        call stiffness(n, AE)
        do j = 1, 3
            do i = 1, 3
                t = t + 1
                ti(t) = ele(i, n)
                tj(t) = ele(j, n)
                tz(t) = AE(i, j)
            enddo
        enddo
        call mass(n, AE)
        tm(t - 8 : t) = reshape(AE, [9])
    enddo

    ! the pattern: a row's columns in the order the stream first names them
    allocate(ptr(nn + 1), deg(nn))
    deg = 0
    do i = 1, nn
        seen = .false.
        do t = 1, 9 * ne
            if (ti(t) == i .and. .not. seen(tj(t))) then
                seen(tj(t)) = .true.
                deg(i) = deg(i) + 1
            endif
        enddo
    enddo
    ptr(1) = 1
    do i = 1, nn
        ptr(i + 1) = ptr(i) + deg(i)
    enddo
    allocate(node(ptr(nn + 1) - 1))
    deg = 0
    do t = 1, 9 * ne
        i = ti(t)
        if (.not. any(node(ptr(i) : ptr(i) + deg(i) - 1) == tj(t))) then
            node(ptr(i) + deg(i)) = tj(t)
            deg(i) = deg(i) + 1
        endif
    enddo

    ! CSR: one batch on the device against the scalar loop on the host mirror
    call Ad%init(nn, nn, ptr, node)
    call Ah%init(nn, nn, ptr, node)
    call Md%init(nn, nn, ptr, node)
    call Ad%add_values_at(ti, tj, tz)
    do t = 1, 9 * ne
        call Ah%add_value(ti(t), tj(t), tz(t))
    enddo
    call check('csr add_values_at = add_value loop', same(Ad%val, Ah%val))
    ! element by element through add_multiple_values; B(k,l) goes to (is(k), js(l))
    call Md%zero()
    do n = 1, ne
        call mass(n, AE)
        call Md%add_multiple_values(ele(:, n), ele(:, n), AE)
    enddo
    call Ah%zero()
    do n = 1, ne
        call mass(n, AE)
        do i = 1, 3
            do j = 1, 3
                call Ah%add_value(ele(i, n), ele(j, n), AE(i, j))
            enddo
        enddo
    enddo
    call check('csr add_multiple_values = add_value loop', same(Md%val, Ah%val))
    call Md%scalar_multiply(0.375_dp)
    Ah%val = 0.375_dp * Ah%val
    call check('csr scalar_multiply', same(Md%val, Ah%val))
    call Md%set_values_at(ti(1:27), tj(1:27), tm(1:27))
    do t = 1, 27
        call Ah%set_value(ti(t), tj(t), tm(t))
    enddo
    call check('csr set_values_at = set_value loop', same(Md%val, Ah%val))

    ! ELLPACK
    call Ed%init(nn, nn, maxval(deg))
    call Eh%init(nn, nn, maxval(deg))
    do t = 1, 9 * ne
        call Ed%add_edge(ti(t), tj(t))
        call Eh%add_edge(ti(t), tj(t))
    enddo
    call Ed%add_values_at(ti, tj, tz)
    do t = 1, 9 * ne
        do k = 1, Eh%degrees(ti(t))
            if (Eh%node(k, ti(t)) == tj(t)) Eh%val(k, ti(t)) = Eh%val(k, ti(t)) + tz(t)
        enddo
    enddo
    call check('ellpack add_values_at = add_value loop', same(reshape(Ed%val, [size(Ed%val)]), reshape(Eh%val, [size(Eh%val)])))
    call Ed%scalar_multiply(-2.5_dp)
    Eh%val = -2.5_dp * Eh%val
    call check('ellpack scalar_multiply', same(reshape(Ed%val, [size(Ed%val)]), reshape(Eh%val, [size(Eh%val)])))

    ! (A + M) u = M 1 with the assembled matrices: the edited handle is a whole matrix
    call Ad%add_values_at(ti, tj, tm)
    allocate(u(nn), b(nn), ones(nn))
    ones = 1.0_dp
    call Md%zero()
    call Md%add_values_at(ti, tj, tm)
    call Md%matvec(ones, b)
    u = 0.0_dp
    solver => hip_cg(1.0e-12_dp)
    call solver%setup(Ad)
    call solver%solve_plain(Ad, u, b)
    call check('cg on the assembled matrix: u = 1', maxval(abs(u - 1.0_dp)) < 1.0e-8_dp)
    print '(a,i0,a,es9.2)', ' cg iterations ', solver%iterations, ', max |u - 1| = ', maxval(abs(u - 1.0_dp))
    call solver%destroy()
    call Ad%destroy()
    call Ah%destroy()
    call Md%destroy()
    call Ed%destroy()
    call Eh%destroy()
    if (fails > 0) then
        print *, 'edit_test_hip: FAILED'
        call exit(1)
    endif
    print *, 'edit_test_hip: ok'

contains

subroutine stiffness(n, AE)
    integer, intent(in) :: n
    real(dp), intent(out) :: AE(3, 3)
    real(dp) :: V(3, 2), det, area
    integer :: i, j, k
    do i = 1, 3
        j = ele(mod(i, 3) + 1, n)
        k = ele(mod(i + 1, 3) + 1, n)
        V(i, 1) = x(2, j) - x(2, k)
        V(i, 2) = x(1, k) - x(1, j)
    enddo
    det = V(1, 1) * V(2, 2) - V(1, 2) * V(2, 1)
    area = abs(det) / 2.0_dp
    AE = 0.25_dp / area * matmul(V, transpose(V))
end subroutine

subroutine mass(n, BE)
    integer, intent(in) :: n
    real(dp), intent(out) :: BE(3, 3)
    real(dp) :: area
    integer :: i, j
    do j = 1, 2
        do i = 1, 2
            BE(i, j) = x(i, ele(j, n)) - x(i, ele(3, n))
        enddo
    enddo
    area = 0.5_dp * abs(BE(1, 1) * BE(2, 2) - BE(1, 2) * BE(2, 1))
    BE = area / 12.0_dp
    do i = 1, 3
        BE(i, i) = area / 6.0_dp
    enddo
end subroutine

logical function same(p, q)
    real(dp), intent(in) :: p(:), q(:)
    same = all(transfer(p, 1_c_int64_t, size(p)) == transfer(q, 1_c_int64_t, size(q)))
end function

subroutine check(what, ok)
    character(len=*), intent(in) :: what
    logical, intent(in) :: ok
    if (ok) then
        print *, 'ok    ', what
    else
        print *, 'FAILED ', what
        fails = fails + 1
    endif
end subroutine

end program edit_test_hip
